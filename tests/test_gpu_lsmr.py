"""-m gpu: `linalg.lstsq` on the HIP kernels (native_lsmr.py) — dense, CSR, banded and generic operators.

Operators are small with a prescribed spectrum (singular values log-spaced in [1 / kappa, 1]): 96 x 40, 40 x 96 and
64 x 64, kappa in {1e2, 1e4}, three columns, a batch of two operators against ONE right-hand side block (broadcast).
MAX_NITER comes from the float64 restatement on the CPU: tests/test_lsmr_ref.py::test_solver_cases_converge_on_the_
restated_iteration asserts that every case below stops on S1 or S2 there within MAX_NITER steps (the slowest takes 999:
64 x 64, kappa = 1e4, atol = 1e-10), so no GPU case may end on max_niter.

Criteria (float64 on the host, from the returned x; |A|_F and sigma_min from the float64 matrix):
  optimality      |A^H (b - A x) - damp^2 x| <= 2 atol |A|_F |rbar|   (the estimate |A| never exceeds |A|_F; 2 is the
                  driver's confirmation margin) for systems that stopped on S2
  forward error   |x - x*| <= 2 atol |A|_F |rbar| / sigma_min(Abar)^2  (x - x* = N^-1 (optimality residual))
  consistent      stop code 1 and |b - A x| <= 2 (btol |b| + atol |A|_F |x|); every system that stopped on S1 is held to
                  that bound (at kappa = 1e4 a wide or square system may meet S2 first: see `expects_s1`)
  minimum norm    |x - P x| / |x| with P the projector on range(A^H), at most 4 times what the host path gives on the
                  CPU in the same dtype (the summation order differs).  Measured CPU values (host path): wide
                  40 x 96, kappa 1e2: f64 1.4e-14, f32 4.1e-6, c128 9.5e-15, c64 3.2e-6; rank 25 of 96 x 40: f64 3.8e-14,
                  f32 1.1e-5, c128 2.5e-14, c64 6.1e-6.
atol = btol = 1e-10 for f64 / c128, 1e-4 for f32 / c64."""
import math
import warnings
import pytest
import torch
from tests import lsmr_ref as lref
from xitorch_amd import LinearOperator
from xitorch_amd._util import ConvergenceWarning
from xitorch_amd.linop import SparseLinearOperator, BandedLinearOperator

DEV = torch.device("cuda:0")
DTYPES, IDS = lref.DTYPES, lref.IDS
SHAPES = [(96, 40), (40, 96), (64, 64)]
KAPPAS = [1e2, 1e4]
MAX_NITER = 4000
NCOLS = 3


def tol_of(dtype):
    return 1e-10 if dtype in (torch.float64, torch.complex128) else 1e-4


def hp_of(dtype):
    return torch.complex128 if dtype.is_complex else torch.float64


def _randn(g, dtype, *shape):
    Z = torch.randn(*shape, dtype=torch.float64, generator=g)
    if dtype.is_complex:
        Z = torch.complex(Z, torch.randn(*shape, dtype=torch.float64, generator=g))
    return Z


def problem(dtype, shape, kappa, consistent=False, rank=None, seed=0):
    """A (2, m, n), B (m, 3) (consistent: (2, m, 3)) in float64 / complex128 (values representable in `dtype`), singular values of both members"""
    m, n = shape
    g = torch.Generator().manual_seed(1000 * m + n + int(math.log10(kappa)) + seed)
    mats = [lref.spectrum_matrix(g, dtype, m, n, kappa, rank=rank)[0] for _ in range(2)]
    A = torch.stack(mats).to(dtype).to(hp_of(dtype))
    if consistent:
        B = A @ _randn(g, dtype, n, NCOLS)                # (2, m, 3): each member its own consistent block
    else:
        B = _randn(g, dtype, m, NCOLS)
    return A, B.to(dtype).to(hp_of(dtype))


def solver_cases():
    """(id, dtype, shape, kappa, consistent, damp) of the dense sweep"""
    out = []
    for d, i in zip(DTYPES, IDS):
        for shape in SHAPES:
            for kappa in KAPPAS:
                out.append(("%s-%dx%d-k%.0e" % (i, shape[0], shape[1], kappa), d, shape, kappa, False, 0.0))
        out.append(("%s-96x40-consistent" % i, d, (96, 40), 1e2, True, 0.0))
        out.append(("%s-96x40-k1e4-damped" % i, d, (96, 40), 1e4, False, 1e-2))
    return out


CASES = solver_cases()


def expects_s1(shape, kappa, consistent, damp):
    """consistent systems stop on S1: the tall case built to be consistent, and the wide and square ones (every b lies
    in the range of a full-row-rank A) — at kappa = 1e2; at kappa = 1e4 the rule S2 (atol |A| |r| with atol kappa up to
    1 in single precision) may be met first, and each system is then held to the rule it stopped on"""
    return damp == 0 and kappa <= 1e2 and (consistent or shape[0] <= shape[1])


def reference(A, B, damp):
    """x* of the stacked problem in float64, |A|_F, sigma_min(Abar) per member"""
    n = A.shape[-1]
    hp = A.dtype
    Ab = torch.cat([A, damp * torch.eye(n, dtype=hp).expand(A.shape[0], n, n)], dim=-2) if damp > 0 else A
    Bb = B.expand(A.shape[0], *B.shape[-2:])
    if damp > 0:
        Bb = torch.cat([Bb, torch.zeros(A.shape[0], n, B.shape[-1], dtype=hp)], dim=-2)
    xs = torch.linalg.pinv(Ab, rtol=1e-13) @ Bb
    sv = torch.linalg.svdvals(Ab)
    return xs, torch.linalg.matrix_norm(A), sv


def criteria(A, B, damp, x, atol, btol, codes, expect_s1=False, rank_full=True):
    """assert the criteria of the module docstring on x (2, n, 3) float64 / complex128, each system by the rule it
    stopped on (`codes`, member-major; expect_s1: every system must have stopped on S1)"""
    xs, fro, sv = reference(A, B, damp)
    Bb = B.expand(A.shape[0], *B.shape[-2:])
    r = Bb - A @ x
    g = A.conj().transpose(-2, -1) @ r - damp * damp * x
    nrm = lambda t: torch.linalg.vector_norm(t, dim=-2)
    nr, ng, nx, nb = nrm(r), nrm(g), nrm(x), nrm(Bb)
    nrbar = torch.sqrt(nr ** 2 + (damp * nx) ** 2)
    F = fro.unsqueeze(-1)
    code = torch.tensor(codes).reshape(nr.shape)
    assert all(c in (1, 2, 4, 5) for c in codes), codes
    if expect_s1:
        assert all(c == 1 for c in codes), codes
    s1 = (code == 1) | (code == 5)
    lim1 = 2 * (btol * nb + atol * F * nx)
    lim2 = 2 * atol * F * nrbar
    if bool(s1.any()):
        print("S1: max |rbar| / bound = %.3e" % float((nrbar / lim1)[s1].max()))
    if bool((~s1).any()):
        print("S2: max |g| / bound = %.3e" % float((ng / lim2)[~s1].max()))
    assert bool((nrbar <= lim1)[s1].all()), (nrbar, lim1, codes)
    assert bool((ng <= lim2)[~s1].all()), (ng, lim2, codes)
    if rank_full and (A.shape[-2] >= A.shape[-1] or damp > 0):
        smin = sv[:, -1:]
        ferr = nrm(x - xs)
        flim = torch.where(s1, lim1 / smin, lim2 / smin ** 2)      # S1: A (x - x*) = r* - r, |x - x*| <= |r| / sigma_min
        print("forward error: max / bound = %.3e" % float((ferr / flim).max()))
        assert bool((ferr <= flim).all()), (ferr, flim)


def outside_range(A, x):
    """|x - P x| / |x| with P the orthogonal projector on range(A^H), float64"""
    P = torch.linalg.pinv(A, rtol=1e-5) @ A      # (singular values below 1e-5: the rounding of a rank-deficient A)
    return float((torch.linalg.vector_norm(x - P @ x, dim=-2) / torch.linalg.vector_norm(x, dim=-2)).max())


def _solve(op, B, dtype, damp=0.0, **kw):
    from xitorch_amd.linalg import lstsq, host_lsmr
    before = host_lsmr.calls["lsmr"]
    trace = {}
    t = tol_of(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        x = lstsq(op, B.to(dtype).to(DEV), damp=damp, atol=t, btol=t, max_niter=MAX_NITER, trace=trace, **kw)
    assert host_lsmr.calls["lsmr"] == before, "a device operator reached the host driver"
    assert trace["niter"] < MAX_NITER and 0 not in trace["stop_codes"]
    every = kw.get("resid_calc_every", 10)
    assert trace["host_reads"] <= trace["niter"] / every + 2 + trace["restarts"], trace
    return x.cpu().to(hp_of(dtype)), trace


def _csr(A):
    """CSR operator on the device from the dense host matrices A (2, m, n) (full pattern, batched values)"""
    m, n = A.shape[-2:]
    crow = torch.arange(0, m * n + 1, n, dtype=torch.int64)
    cols = torch.arange(n, dtype=torch.int64).repeat(m)
    return SparseLinearOperator(crow.to(DEV), cols.to(DEV), A.reshape(A.shape[0], m * n).to(DEV), (A.shape[0], m, n))


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


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dense(case):
    _, dtype, shape, kappa, consistent, damp = case
    A, B = problem(dtype, shape, kappa, consistent=consistent)
    x, trace = _solve(LinearOperator.m(A.to(dtype).to(DEV)), B, dtype, damp=damp)
    assert trace["panel_kernel"] == "dense" and trace["torch_applies"] == 0
    t = tol_of(dtype)
    criteria(A, B, damp, x, t, t, trace["stop_codes"], expect_s1=expects_s1(shape, kappa, consistent, damp))


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex64], ids=["f64", "c64"])
@pytest.mark.parametrize("shape", [(96, 40), (40, 96)], ids=["tall", "wide"])
def test_csr(dtype, shape):
    A, B = problem(dtype, shape, 1e2)
    x, trace = _solve(_csr(A.to(dtype)), B, dtype)
    assert trace["panel_kernel"] == "csr" and trace["torch_applies"] == 0
    t = tol_of(dtype)
    criteria(A, B, 0.0, x, t, t, trace["stop_codes"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_banded_square_nonsymmetric(dtype):
    g = torch.Generator().manual_seed(5)
    N, hb = 64, 2
    band = 0.3 * torch.randn(2, 2 * hb + 1, N, dtype=torch.float64, generator=g)
    band[:, hb] = 2.0 + torch.rand(2, N, dtype=torch.float64, generator=g)          # dominant diagonal: kappa < 10
    band = band.to(dtype)
    op = BandedLinearOperator(band.to(DEV))
    A = op.fullmatrix().cpu().to(torch.float64)
    assert float((A - A.transpose(-2, -1)).abs().max()) > 0.1
    B = torch.randn(N, NCOLS, dtype=torch.float64, generator=g).to(dtype).to(torch.float64)
    x, trace = _solve(op, B, dtype)
    assert trace["panel_kernel"] == "banded" and trace["torch_applies"] == 0
    t = tol_of(dtype)
    criteria(A, B, 0.0, x, t, t, trace["stop_codes"])


def test_generic_operator():
    dtype = torch.float64
    A, B = problem(dtype, (40, 96), 1e2)
    x, trace = _solve(_Generic(A.to(DEV)), B, dtype)
    assert trace["panel_kernel"] == "generic" and trace["torch_applies"] == trace["napply"]
    criteria(A, B, 0.0, x, 1e-10, 1e-10, trace["stop_codes"], expect_s1=True)


def test_batched_rhs_against_one_operator_and_resid_calc_every():
    dtype = torch.float64
    A, B = problem(dtype, (96, 40), 1e2)
    g = torch.Generator().manual_seed(9)
    B2 = torch.randn(2, 96, NCOLS, dtype=torch.float64, generator=g)
    x, trace = _solve(LinearOperator.m(A[0].to(DEV)), B2, dtype, resid_calc_every=3)
    xs = torch.linalg.lstsq(A[0].expand(2, 96, 40), B2).solution
    assert float((x - xs).abs().max()) <= 1e-8 * float(xs.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["wide", "rank-deficient"])
def test_minimum_norm(dtype, kind):
    from xitorch_amd.linalg import lstsq
    if kind == "wide":
        A, B = problem(dtype, (40, 96), 1e2)
    else:
        A, B = problem(dtype, (96, 40), 1e2, rank=25)
    x, trace = _solve(LinearOperator.m(A.to(dtype).to(DEV)), B, dtype)
    t = tol_of(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        xh = lstsq(LinearOperator.m(A.to(dtype)), B.to(dtype), atol=t, btol=t, max_niter=MAX_NITER)
    cpu = outside_range(A, xh.to(hp_of(dtype)))
    gpu = outside_range(A, x)
    print("outside range(A^H): host path %.3e, kernels %.3e (%s, %s)" % (cpu, gpu, dtype, kind))
    assert gpu <= 4 * cpu, (gpu, cpu)
    criteria(A, B, 0.0, x, t, t, trace["stop_codes"], expect_s1=(kind == "wide"), rank_full=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_damped_against_the_closed_form(dtype):
    damp = 1e-2
    A, B = problem(dtype, (96, 40), 1e4)
    x, trace = _solve(LinearOperator.m(A.to(dtype).to(DEV)), B, dtype, damp=damp)
    AH = A.conj().transpose(-2, -1)
    N = AH @ A + damp * damp * torch.eye(40, dtype=A.dtype)
    xs = torch.linalg.solve(N, AH @ B.expand(2, 96, NCOLS))
    t = tol_of(dtype)
    fro = torch.linalg.matrix_norm(A).unsqueeze(-1)
    r = B - A @ x
    nrbar = torch.sqrt(torch.linalg.vector_norm(r, dim=-2) ** 2 + (damp * torch.linalg.vector_norm(x, dim=-2)) ** 2)
    smin2 = torch.linalg.eigvalsh(N)[:, :1]
    err = torch.linalg.vector_norm(x - xs, dim=-2)
    lim = 2 * t * fro * nrbar / smin2
    print("damped: max err / bound = %.3e" % float((err / lim).max()))
    assert bool((err <= lim).all()), (err, lim)


def test_conlim_warns():
    from xitorch_amd.linalg import lstsq
    A, B = problem(torch.float64, (96, 40), 1e4)
    with pytest.warns(ConvergenceWarning, match="regularised"):
        lstsq(LinearOperator.m(A.to(DEV)), B.to(DEV), atol=1e-14, btol=1e-14, conlim=50.0, max_niter=MAX_NITER)


def _loss_weights(g, dtype, *shape):
    return _randn(g, dtype, *shape)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["f64", "c128"])
@pytest.mark.parametrize("shape,damp", [((96, 40), 0.0), ((40, 96), 0.0), ((40, 96), 1e-1)],
                         ids=["column-rank", "row-rank", "wide-damped"])
@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_backward(dtype, shape, damp, kind):
    """gradients with respect to B and the values of A against torch.linalg.lstsq / the closed form under autograd on
    the CPU in float64.  Tolerance: the forward-error bound applied to the backward solves — each of the two solves is
    accurate to 2 atol |A|_F |rbar| / sigma_min^2 relative to its right-hand side's scale, and the VJPs are bilinear
    in (w, r) / (x, A w): TOL = 8 atol kappa^2 relative to the largest gradient entry."""
    from xitorch_amd.linalg import lstsq
    m, n = shape
    kappa = 1e2
    A, B = problem(dtype, shape, kappa)
    A, B = A[0], B
    g = torch.Generator().manual_seed(3)
    W = _loss_weights(g, dtype, n, NCOLS)
    t = tol_of(dtype)
    Ac = A.clone().requires_grad_()
    Bc = B.clone().requires_grad_()
    if damp > 0:
        AH = Ac.conj().transpose(-2, -1)
        xc = torch.linalg.solve(AH @ Ac + damp * damp * torch.eye(n, dtype=A.dtype), AH @ Bc)
    else:
        xc = torch.linalg.pinv(Ac) @ Bc
    (xc * W.conj()).real.sum().backward()
    Ad = A.to(DEV).requires_grad_()
    Bd = B.to(DEV).requires_grad_()
    if kind == "dense":
        op = LinearOperator.m(Ad)
        vals = Ad
    else:
        crow = torch.arange(0, m * n + 1, n, dtype=torch.int64, device=DEV)
        cols = torch.arange(n, dtype=torch.int64, device=DEV).repeat(m)
        vals = A.reshape(m * n).to(DEV).requires_grad_()
        op = SparseLinearOperator(crow, cols, vals, (m, n))
    x = lstsq(op, Bd, damp=damp, atol=t, btol=t, max_niter=MAX_NITER)
    (x * W.conj().to(DEV)).real.sum().backward()
    tol = 8 * t * kappa ** 2
    gA = vals.grad.cpu().reshape(m, n)
    for got, want, name in ((Bd.grad.cpu(), Bc.grad, "B"), (gA, Ac.grad, "A")):
        err = float((got - want).abs().max()) / float(want.abs().max())
        print("backward %s: relative error %.3e (tolerance %.3e)" % (name, err, tol))
        assert err <= tol, (name, err, tol)
