"""-m gpu: funm_multiply / expm_multiply on the HIP kernels (native_fnm.py) — dense, CSR, banded and user operators.

The cases and gates are those of tests/test_host_fnm.py, against the same dense truth and the same restatement; every
device result is also set beside the host result of the same call: both are held to the gate against the truth, and
their difference to the same gate once (4 x the restatement's error + 16 n eps_T), not to the two gates' sum.  A device operator never reaches the host driver, and two runs give
identical bits.  Shapes are no larger than n = 257, p = 3, batch 2."""
import numpy as np
import pytest
import torch
from tests import fnm_ref as fref
from tests import test_host_fnm as H
from tests.test_gpu_slq_kernels import _same
from xitorch_amd import LinearOperator
from xitorch_amd.linalg import funm_multiply, host_slq

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _host_driver_is_not_reached():
    before = host_slq.calls["funm"]
    H_calls = []
    yield H_calls
    assert host_slq.calls["funm"] == before + sum(H_calls), "a device operator reached the host driver"


@pytest.mark.parametrize("n,nsteps", H.SHAPES)
@pytest.mark.parametrize("kind,dtype", H.KINDS, ids=H.KIND_IDS)
def test_against_truth(kind, dtype, n, nsteps, _host_driver_is_not_reached):
    op, _ = H.operators(kind, dtype, n, DEV)
    got = H.check_against_restatement(op, kind, dtype, n, nsteps, "device %s %s" % (kind, dtype))
    # the host call on the same input: the two results differ by no more than ONE gate (each is within a gate of the
    # truth, which alone would allow two)
    hop, _ = H.operators(kind, dtype, n)
    A, B, truth, referr = H.problem(kind, dtype, n, nsteps)
    eps = torch.finfo(dtype).eps
    for name, (fn, t, _) in H.FUNCS.items():
        Xh = funm_multiply(hop, B, fn, nsteps=nsteps, t=t)
        _host_driver_is_not_reached.append(1)
        diff = H.colerr(got[name], Xh.to(truth[name].dtype))
        print("device - host %s %s %s n=%d nsteps=%d: %s" % (kind, dtype, name, n, nsteps,
                                                             " ".join("%.2e" % d for d in diff)))
        assert all(d <= 4 * r + 16 * n * eps for d, r in zip(diff, referr[name])), (name, diff)
    # two runs: identical bits
    again = funm_multiply(op, B.to(DEV), "sqrt", nsteps=nsteps)
    _same(again, got["sqrt"], "second run")


def test_larger_than_one_block_of_rows():
    """n = 257 (odd, beyond the 256 threads of a block), batch 2, p = 3, float32 and complex128"""
    n, nsteps = 257, 30
    for dtype in (torch.float32, torch.complex128):
        A, Q, lam = H.hermitian(n, dtype, kappa=4.0)
        Ad = torch.stack([A, 2 * A]).to(dtype)
        op = LinearOperator.m(Ad.to(DEV), is_hermitian=True)
        B = H.rhs(n, 3, dtype)
        tr = {}
        X = funm_multiply(op, B.to(DEV), "invsqrt", nsteps=nsteps, trace=tr)
        assert X.shape == (2, n, 3) and tr["nsteps"].tolist() == [[nsteps] * 3] * 2 and tr["napply"] == 2 * nsteps - 1
        eps = torch.finfo(dtype).eps
        for bi in range(2):
            An = Ad[bi].to(A.dtype).numpy()
            An = (An + An.conj().T) / 2
            f = lambda x: 1 / np.sqrt(x)
            for j in range(3):
                bj = B[:, j].to(A.dtype).numpy()
                want = fref.dense_truth(An, bj, f)
                xr, _, _ = fref.funm(An, bj, nsteps, f, fref.ARITH[dtype])
                referr = np.linalg.norm(xr - want) / np.linalg.norm(want)
                err = np.linalg.norm(X[bi, :, j].cpu().to(A.dtype).numpy() - want) / np.linalg.norm(want)
                print("n=257 %s member %d column %d: error %.2e, restatement %.2e" % (dtype, bi, j, err, referr))
                assert err <= 4 * referr + 16 * n * eps


def test_batch_broadcasting():
    H.test_batch_broadcasting(DEV)


def test_expm_multiply_both_signs():
    H.test_expm_multiply_both_signs(DEV)


def test_complex_callable_against_eigh():
    H.test_complex_callable_against_eigh(DEV)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_breakdown_is_exact(dtype):
    H.test_breakdown_is_exact(dtype, DEV)


def test_zero_column():
    H.test_zero_column(DEV)


def test_indefinite_member_is_nan_with_one_warning():
    H.test_indefinite_member_is_nan_with_one_warning(DEV)


def test_rtol_warning():
    H.test_rtol_warning(DEV)


@pytest.mark.parametrize("dtype", H.DTYPES[:2], ids=H.IDS[:2])
def test_gradient_with_respect_to_B(dtype):
    """the backward is one more device call with the conjugated function: against the dense expression"""
    n = 12
    A, Q, lam = H.hermitian(n, dtype, kappa=4.0)
    op = LinearOperator.m(A.to(DEV), is_hermitian=True)
    B = H.rhs(n, 2, dtype).to(DEV).requires_grad_()
    G = H.rhs(n, 2, dtype, seed=5).to(DEV)
    f = (lambda x: torch.exp(-0.5j * x)) if dtype.is_complex else torch.rsqrt
    X = funm_multiply(op, B, f, nsteps=n)
    gB, = torch.autograd.grad(X, B, G)
    want = (Q * torch.conj(f(lam.to(A.dtype)))) @ (Q.conj().T @ G.cpu())
    assert float((gB.cpu() - want).norm() / want.norm()) <= 16 * n * 2.0 ** -52
