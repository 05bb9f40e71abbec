"""-m gpu: fsai_lu() through the drivers on the device — the "fsai_lu" panel kind (two xk_csr_mm launches for P and for
P^H, no torch-expression apply), gmres(precond_r=) for float64 and complex128, bicgstab with the named preconditioner,
the string forwards and backwards through solve(), the equality with fsai() on a Hermitian positive definite operator,
and the unpreconditioned gmres left as it was.

The problem is the convection-diffusion grid of tests/fsai_lu_cases.py at n = 24, pe = 0.5 (order 576, kappa_2 = 317):
un-restarted GMRES to a relative true residual of 1e-8 needs about 103 Arnoldi steps without a preconditioner and about
43 / 30 with fsai_lu(A, power=1 / 2) (tests/test_host_fsai_lu.py runs the same on the host); the complex problem is the
same operator times a unit-modulus diagonal plus 0.1i on the diagonal."""
import hashlib
import warnings
import numpy as np
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import linop
from xitorch_amd.linop import SparseLinearOperator
from xitorch_amd.linalg import solve, fsai, fsai_lu, host_krylov, native_krylov
from xitorch_amd.linalg import precond as precond_mod
from xitorch_amd.linalg._panel import PanelOperator, pad_len
from tests import fsai_cases as fc
from tests import fsai_lu_cases as lc

pytestmark = pytest.mark.gpu
n = 24
N = n * n
F64, C128 = torch.float64, torch.complex128
RTOL = 1e-8


def _boom(*a, **k):
    raise AssertionError("torch-expression apply on the device path")


def _no_torch_apply(monkeypatch):
    monkeypatch.setattr(linop, "csr_apply_torch", _boom)
    for cls in (linop.SparseLinearOperator, precond_mod.FSAILUOperator):
        for name in ("_mm", "_mv", "_rmm", "_rmv"):
            monkeypatch.setattr(cls, name, _boom)


@pytest.fixture(scope="module")
def problems():
    """dense matrices (float64, complex128) and right-hand sides, built once"""
    Ad = lc.convdiff(n, 0.5)
    Ac = lc.convdiff_complex(n, 0.5)
    b = lc.convdiff_rhs(N, 2)
    bc = b + 1j * np.random.default_rng(3).standard_normal((N, 2))
    return {F64: (Ad, torch.as_tensor(b)), C128: (Ac, torch.as_tensor(bc))}


def _relres(Ad, X, B):
    Ad = torch.as_tensor(Ad)
    return float(((Ad @ X.cpu().to(Ad.dtype) - B.cpu()).norm(dim=-2) / B.cpu().norm(dim=-2)).max())


def _gmres(A, B, must_converge=True, **kw):
    tr = {}
    before = dict(host_krylov.calls)
    with warnings.catch_warnings():
        warnings.simplefilter("error" if must_converge else "ignore", xa.ConvergenceWarning)
        X = native_krylov.gmres(A, B, rtol=RTOL, atol=0.0, posdef=True, trace=tr, **kw)
    assert host_krylov.calls == before, "a device run reached a host driver"
    assert tr["converged"] or not must_converge
    return X, tr


@pytest.mark.parametrize("dtype", [F64, C128])
def test_panel_kind_applies_p_and_its_adjoint(dev, dtype, problems, monkeypatch):
    Ad, _ = problems[dtype]
    Ab = np.stack([Ad, Ad * 1.5])
    A = lc.operator_of_dense(Ab, device=dev)
    P = fsai_lu(A)
    assert P.device.type == "cuda" and P.dtype == dtype and int(P.nfallback.sum()) == 0
    GL, GU = lc.factors_dense(P)
    Pd = torch.as_tensor(GU @ GL)
    absP = torch.as_tensor(np.abs(GU) @ np.abs(GL))
    ld = pad_len(N)
    g = torch.Generator().manual_seed(3)
    eps = torch.finfo(dtype).eps
    for op_, dense_ in ((P, Pd), (P.H, Pd.mH)):
        op = PanelOperator(op_, [2], 2, N)
        assert op.kind == "fsai_lu" and op.pat._csc is not None, "the CSC view is built with the operator"
        for trans in (False, True):
            want = dense_.mH if trans else dense_
            mag_op = absP.mT if (trans != (op_ is not P)) else absP
            for p in (1, 3, 9, 3):
                X = torch.zeros((2, p, ld), dtype=dtype, device=dev)
                X[:, :, :N] = torch.randn(2, p, N, dtype=torch.float64, generator=g).to(dtype).to(dev)
                scr = op._scratch
                out = torch.full_like(X, 7.0)
                _no_torch_apply(monkeypatch)
                op.apply(X, out, trans=trans)
                monkeypatch.undo()
                assert op.last_kernel == "fsai_lu" and op.torch_applies == 0
                if scr is not None and scr.shape[1] >= p:
                    assert op._scratch is scr, "the scratch panel is reallocated only when the column count grows"
                assert bool((out[:, :, N:] == 7.0).all()), "pads are not written"
                xc = X[:, :, :N].cpu().transpose(-2, -1)
                ref = (want @ xc).transpose(-2, -1)
                mag = (mag_op @ xc.abs()).transpose(-2, -1)
                assert bool(((out[:, :, :N].cpu() - ref).abs() <= 32 * eps * mag).all())


@pytest.mark.parametrize("dtype", [F64, C128])
def test_gmres_halves_the_steps_and_matches_the_host(dev, dtype, problems, monkeypatch):
    Ad, B = problems[dtype]
    A = lc.operator_of_dense(Ad, device=dev)
    Bd = B[:, :1].to(dev)
    # the plain run: 103 steps for the real problem; the complex one (eigenvalues all around the origin) is not solved
    # within 240 steps, which is then the count the preconditioned runs are held against
    X0, tr0 = _gmres(A, Bd, must_converge=not dtype.is_complex, max_niter=241)
    assert tr0["converged"] == (not dtype.is_complex)
    P1, P2 = fsai_lu(A), fsai_lu(A, power=2)
    assert int(P1.nfallback) == 0 and int(P2.nfallback) == 0
    # the operators the driver builds report which kernels served them
    made = []
    real = native_krylov.PanelOperator

    def spy(*a, **k):
        made.append(real(*a, **k))
        return made[-1]
    monkeypatch.setattr(native_krylov, "PanelOperator", spy)
    _no_torch_apply(monkeypatch)
    X1, tr1 = _gmres(A, Bd, precond_r=P1)
    monkeypatch.undo()
    kinds = {op.kind: op for op in made}
    assert set(kinds) == {"csr", "fsai_lu"}
    assert kinds["fsai_lu"].last_kernel == "fsai_lu" and kinds["csr"].last_kernel == "csr"
    assert kinds["fsai_lu"].torch_applies == 0 and kinds["csr"].torch_applies == 0
    assert kinds["fsai_lu"].napply >= tr1["arnoldi_steps"]
    X2, tr2 = _gmres(A, Bd, precond_r=P2)
    s0, s1, s2 = tr0["arnoldi_steps"], tr1["arnoldi_steps"], tr2["arnoldi_steps"]
    print("%s gmres Arnoldi steps to 1e-8 on the device: plain %d, fsai_lu(power=1) %d, fsai_lu(power=2) %d"
          % (dtype, s0, s1, s2))
    assert 2 * s1 <= s0 and s2 <= s1
    for X in (X1, X2) + ((X0,) if tr0["converged"] else ()):
        assert _relres(Ad, X, Bd) <= RTOL
    # the host path on the same problem: the same solution within 10 rtol |x|
    Ah = lc.operator_of_dense(Ad)
    Ph = fsai_lu(Ah)
    Xh = host_krylov.gmres(Ah, B[:, :1], rtol=RTOL, atol=0.0, posdef=True, precond_r=Ph)
    assert float((X1.cpu() - Xh).norm()) <= 10 * RTOL * float(Xh.norm())


def test_gmres_options(dev, problems):
    Ad, B = problems[F64]
    A = lc.operator_of_dense(Ad, device=dev)
    P = fsai_lu(A)
    Bd = B.to(dev)
    # GMRES(20) within 100 steps (the plain restarted run needs about 160: tests/test_host_fsai_lu.py)
    X, tr = _gmres(A, Bd[:, :1], precond_r=P, restart=20, max_niter=100)
    assert tr["restarts"] >= 1 and _relres(Ad, X, Bd[:, :1]) <= RTOL
    with pytest.warns(xa.ConvergenceWarning):
        native_krylov.gmres(A, Bd[:, :1], rtol=RTOL, atol=0.0, posdef=True, restart=20, max_niter=100)
    # true residuals every fifth step only
    X, tr5 = _gmres(A, Bd[:, :1], precond_r=P, resid_calc_every=5)
    assert _relres(Ad, X, Bd[:, :1]) <= RTOL
    # per-column shifts and two columns
    E = torch.tensor([-0.3, 0.05], dtype=F64, device=dev)
    X, _ = _gmres(A, Bd, E=E, precond_r=P)
    for c in range(2):
        r = (torch.as_tensor(Ad) - float(E[c]) * torch.eye(N, dtype=F64)) @ X[:, c].cpu() - B[:, c]
        assert float(r.norm() / B[:, c].norm()) <= RTOL
    # a batch of two operators with different values, two columns
    Ab = np.stack([Ad, lc.convdiff(n, 1.0)])
    A2 = lc.operator_of_dense(Ab, device=dev)
    P2 = fsai_lu(A2)
    assert not torch.equal(P2.GL.values[0], P2.GL.values[1])
    Xb, trb = _gmres(A2, Bd, precond_r=P2)
    assert Xb.shape == (2, N, 2) and trb["arnoldi_steps"] <= 60
    for b in range(2):
        assert _relres(Ab[b], Xb[b], Bd) <= RTOL
    # the normal equations are refused
    with pytest.raises(ValueError, match="normal equations"):
        native_krylov.gmres(A, Bd, posdef=False, precond_r=P)


def test_bicgstab_with_the_name(dev, problems):
    Ad, B = problems[F64]
    A = lc.operator_of_dense(Ad, device=dev)
    Bd = B.to(dev)
    before = dict(host_krylov.calls)
    tr, tr0 = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(A, Bd, method="bicgstab", precond_r="fsai_lu", rtol=RTOL, atol=0.0, posdef=True, trace=tr)
        Xl = solve(A, Bd, method="bicgstab", precond_l="fsai_lu", rtol=RTOL, atol=0.0, posdef=True)
        solve(A, Bd, method="bicgstab", rtol=RTOL, atol=0.0, posdef=True, trace=tr0)
    assert host_krylov.calls == before
    assert _relres(Ad, X, Bd) <= 2 * RTOL and _relres(Ad, Xl, Bd) <= 2 * RTOL
    assert tr["niter"] < tr0["niter"]


@pytest.mark.parametrize("dtype", [F64, C128])
def test_solve_forward_and_backward_against_exactsolve(dev, dtype):
    m = 8
    Ad = lc.convdiff_complex(m, 0.5) if dtype.is_complex else lc.convdiff(m, 0.5)
    crow, col, vals = lc.csr_of_dense(Ad)
    crow_t, col_t = torch.as_tensor(crow).to(dev), torch.as_tensor(col).to(dev)
    b0 = torch.as_tensor(lc.convdiff_rhs(m * m, 2)).to(dtype).to(dev)
    opts = dict(method="gmres", precond_r="fsai_lu", rtol=1e-13, atol=1e-15, posdef=True)
    outs = []
    before = dict(host_krylov.calls)
    for kw in (dict(bck_options=dict(opts), **opts), dict(method="exactsolve")):
        v = torch.as_tensor(vals).to(dev).requires_grad_()
        b = b0.clone().requires_grad_()
        A = SparseLinearOperator(crow_t, col_t, v, (m * m, m * m))
        x = solve(A, b, **kw)
        outs.append((x.detach(), *torch.autograd.grad((x.abs() ** 2).sum(), (v, b))))
    assert host_krylov.calls == before
    (x1, gv1, gb1), (x0, gv0, gb0) = outs
    assert torch.allclose(x1, x0, rtol=1e-9, atol=1e-11)
    assert torch.allclose(gv1, gv0, rtol=1e-8, atol=1e-10)
    assert torch.allclose(gb1, gb0, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("phase", [False, True])
def test_equals_fsai_on_a_hermitian_positive_definite_operator(dev, phase):
    dtype = C128 if phase else F64
    A, dense = fc.grid_operator(10, nmembers=2, dtype=dtype, device=dev, phase=phase)
    P, Plu = fsai(A), fsai_lu(A)
    assert int(Plu.nfallback.sum()) == 0
    eye = torch.eye(100, dtype=dtype, device=dev).expand(2, 100, 100)
    Pd, Plud = P.mm(eye).cpu().numpy(), Plu.mm(eye).cpu().numpy()
    eps = torch.finfo(dtype).eps
    for b in range(2):
        assert np.abs(Pd[b] - Plud[b]).max() <= 64 * eps * np.linalg.cond(dense[b]) * np.linalg.norm(Pd[b], 2)


# sha256 of the solution bytes of the run below as the commit before gmres(precond_r=) produced them on an MI355X
# (recorded there from a build of that commit, in the same job as this tree's run, which gave the same digests)
PARENT_DIGEST = {
    "torch.float64": "c14b82a2080b8d27a1a3611669fa62cecc4f1498baf1822d3c09bdfa0e4c4bc4",
    "torch.complex128": "f67d5eeb7002f3ddbc73c47b6de90f1529fd4fdae2336f6c3ebdd2eb152d3bf1",
}


def unpreconditioned_reference_run(dev, dtype):
    """the fixed unpreconditioned run whose bits must not change: restarted and un-restarted, two columns, a shift"""
    Ad = lc.convdiff_complex(12, 0.5) if dtype.is_complex else lc.convdiff(12, 0.5)
    A = lc.operator_of_dense(Ad, device=dev)
    B = torch.as_tensor(lc.convdiff_rhs(144, 2)).to(dtype).to(dev)
    E = torch.tensor([-0.3, 0.05], dtype=dtype, device=dev)
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", xa.ConvergenceWarning)       # (the complex runs end at the order, unconverged)
        for kw in (dict(), dict(restart=15, resid_calc_every=4), dict(E=E)):
            outs.append(native_krylov.gmres(A, B, rtol=1e-10, atol=0.0, posdef=True, **kw).contiguous().cpu())
    raw = b"".join(o.numpy().tobytes() for o in outs)
    return outs, hashlib.sha256(raw).hexdigest()


@pytest.mark.parametrize("dtype", [F64, C128])
def test_unpreconditioned_gmres_is_unchanged(dev, dtype):
    outs, digest = unpreconditioned_reference_run(dev, dtype)
    outs2, digest2 = unpreconditioned_reference_run(dev, dtype)
    assert digest == digest2, "the run is not reproducible"
    # precond_r=None is the call without the option
    Ad = lc.convdiff_complex(12, 0.5) if dtype.is_complex else lc.convdiff(12, 0.5)
    A = lc.operator_of_dense(Ad, device=dev)
    B = torch.as_tensor(lc.convdiff_rhs(144, 2)).to(dtype).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", xa.ConvergenceWarning)
        x = native_krylov.gmres(A, B, rtol=1e-10, atol=0.0, posdef=True, precond_r=None)
    assert torch.equal(x.cpu(), outs[0])
    print("unpreconditioned gmres digest %s: %s" % (dtype, digest))
    assert digest == PARENT_DIGEST[str(dtype)], "the bits of the commit before precond_r"
