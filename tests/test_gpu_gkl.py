"""-m gpu: svd(method="gkl") on the HIP kernels (native_gkl.gkl) — the solver cases of tests/test_host_gkl.py on device
operators of every kind, checked by the a-posteriori bounds of tests/gkl_cases.py (true residual, Weyl, orthonormality)."""
import numpy as np
import pytest
import torch
from tests import gkl_cases as gc
from xitorch_amd import LinearOperator
from xitorch_amd.linop import SparseLinearOperator, BandedLinearOperator
from xitorch_amd.linalg import svd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]


def _cast(A64, dtype):
    return A64.to(dtype)


def _run(A, k, mode, ncv=None, op=None, **opts):
    ur = gc.unit_roundoff(A.dtype)
    min_eps = 100 * ur
    trace = {}
    op = LinearOperator.m(A.to(DEV)) if op is None else op
    u, s, vh = svd(op, k=k, mode=mode, method="gkl", min_eps=min_eps, ncv=ncv, trace=trace, **opts)
    assert trace["converged"]
    gc.check(A, u, s, vh, k, mode, min_eps, trace["ncv"], label="%s %s %s" % (tuple(A.shape), A.dtype, mode))
    return trace, (u, s, vh)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(300, 200), (200, 300), (257, 257)])
def test_graded_spectrum(dtype, shape):
    A = _cast(gc.graded(*shape, cplx=dtype.is_complex), dtype)
    trace, _ = _run(A, 10, "uppest")
    assert trace["panel_kernel"] == "dense" and trace["torch_applies"] == 0
    assert trace["host_reads"] == trace["niter"] + len(trace["breakdowns"])      # one status read per cycle


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(400, 260), (260, 400)])
def test_slow_spectrum_restarts(dtype, shape):
    A = _cast(gc.slow(*shape, cplx=dtype.is_complex), dtype)
    trace, _ = _run(A, 6, "uppest", ncv=14)
    assert trace["restarts"] >= 2
    assert trace["host_reads"] == trace["niter"] + len(trace["breakdowns"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(120, 80), (80, 120), (96, 96)])
def test_lowest(dtype, shape):
    A = _cast(gc.lowest(*shape, cplx=dtype.is_complex), dtype)
    trace, (u, s, vh) = _run(A, 3, "lowest")
    assert trace["tall"] == (shape[0] >= shape[1])


def test_dense_crossing_tile_seams():
    A = gc.with_spectrum(1027, 515, np.linspace(1.0, 0.01, 515) ** 3, seed=5)
    _run(A, 5, "uppest")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_with_uneven_convergence(dtype):
    trace, _ = _run(_cast(gc.uneven_batch(cplx=dtype.is_complex), dtype), 4, "uppest", ncv=12)
    gc.check_uneven(trace, 4)


def _csr(A):
    """CSR operator on the device from the non-zeros of the dense host matrix A"""
    rows, cols = torch.nonzero(A, as_tuple=True)                       # row-major order: sorted by row
    crow = torch.zeros(A.shape[0] + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=A.shape[0]), 0)
    return SparseLinearOperator(crow.to(DEV), cols.to(DEV), A[rows, cols].to(DEV), tuple(A.shape))


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["f64", "c128"])
def test_csr_rectangular(dtype):
    rng = np.random.default_rng(11)
    m, n = 515, 259
    dense = rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.05)
    if dtype.is_complex:
        dense = dense + 1j * rng.standard_normal((m, n)) * (dense != 0)
    A = torch.from_numpy(dense).to(dtype)
    trace, _ = _run(A, 4, "uppest", op=_csr(A))
    assert trace["panel_kernel"] == "csr" and trace["torch_applies"] == 0
    At = A.T.contiguous()
    _run(At, 4, "uppest", op=_csr(At))


def test_banded():
    rng = np.random.default_rng(13)
    N, hb = 300, 2
    band = torch.from_numpy(rng.standard_normal((2 * hb + 1, N)))
    op = BandedLinearOperator(band.to(DEV))
    A = op.fullmatrix().cpu()
    trace, _ = _run(A, 4, "uppest", op=op)
    assert trace["panel_kernel"] == "banded" and trace["torch_applies"] == 0


class _Generic(LinearOperator):
    def __init__(self, mat):
        super().__init__(shape=mat.shape, dtype=mat.dtype, device=mat.device)
        self.mat = mat

    def _mv(self, x):
        return torch.matmul(self.mat, x.unsqueeze(-1)).squeeze(-1)

    def _rmv(self, x):
        return torch.matmul(self.mat.transpose(-2, -1).conj(), x.unsqueeze(-1)).squeeze(-1)

    def _getparamnames(self, prefix=""):
        return [prefix + "mat"]


def test_generic_operator():
    A = gc.graded(200, 300)
    trace, _ = _run(A, 6, "uppest", op=_Generic(A.to(DEV)))
    assert trace["panel_kernel"] == "generic" and trace["torch_applies"] == trace["napply"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rank_deficient(dtype):
    """rank 12 below the basis size 20: the Krylov space is exhausted inside the first cycle; whether the norm left by
    the roundings is below u sigma_max (a flagged breakdown) or just above it (a noise vector, orthogonal to the basis
    all the same), the triplets must pass the checks"""
    _run(_cast(gc.rank_deficient(120, 90, 12, cplx=dtype.is_complex), dtype), 5, "uppest")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_breakdown_from_v0(dtype):
    """a diagonal operator started on e_1: A^H u_1 - alpha_1 v_1 is exactly zero, a certain breakdown at the first beta;
    the member continues from a random vector"""
    d = np.linspace(1.0, 0.05, 90) ** 2
    A = torch.zeros((120, 90), dtype=dtype)
    A[torch.arange(90), torch.arange(90)] = torch.from_numpy(d).to(dtype)
    V0 = torch.zeros((90, 1), dtype=dtype)
    V0[0, 0] = 1.0
    trace, _ = _run(A, 5, "uppest", V0=V0.to(DEV))
    assert trace["breakdowns"] and trace["breakdowns"][0][0] == 1
    assert trace["host_reads"] == trace["niter"] + len(trace["breakdowns"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_v0_start(dtype):
    A = _cast(gc.slow(400, 260, cplx=dtype.is_complex), dtype)
    V0 = torch.linalg.svd(A)[2][:6].transpose(0, 1).conj().contiguous()           # the wanted right singular vectors
    cold, _ = _run(A, 6, "uppest", ncv=14)
    warm, _ = _run(A, 6, "uppest", ncv=14, V0=V0.to(DEV))
    assert warm["niter"] <= cold["niter"]


def test_refusals():
    op = LinearOperator.m(gc.graded(300, 200).to(DEV))
    with pytest.raises(NotImplementedError):
        svd(op, k=4, method="gkl", process_group=object())
    with pytest.raises(ValueError):
        svd(op, k=4, method="gkl", ncv=65)
    with pytest.raises(ValueError):
        svd(op, k=20, method="gkl", ncv=20)


@pytest.mark.parametrize("shape", [(40, 24), (24, 40)])
def test_minres_backward_against_dense_autograd(shape):
    torch.manual_seed(3)
    s = np.linspace(2.0, 0.2, min(shape))
    A0 = gc.with_spectrum(*shape, s, seed=17)
    w = torch.linspace(1.0, 2.0, 3, dtype=torch.float64)

    def loss_of(u, sv, vh):
        return sv.sum() + ((u * w.to(u.device)) @ vh).abs().pow(2).sum().sqrt() + (u[..., :, -1:] @ vh[..., -1:, :])[0, 1]

    Ad = A0.clone().to(DEV).requires_grad_()
    u, sv, vh = svd(LinearOperator.m(Ad), k=3, mode="uppest", method="gkl", min_eps=1e-13, ncv=20,
                    bck_options={"method": "minres", "rtol": 1e-12, "atol": 1e-14})
    loss_of(u, sv, vh).backward()
    Ar = A0.clone().requires_grad_()
    U, S, Vh = torch.linalg.svd(Ar, full_matrices=False)
    idx = torch.tensor([2, 1, 0])
    loss_of(U[:, idx], S[idx], Vh[idx]).backward()
    assert (Ad.grad.cpu() - Ar.grad).abs().max() <= 1e-8 * Ar.grad.abs().max()
