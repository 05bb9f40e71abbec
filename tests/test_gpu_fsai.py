"""-m gpu: fsai() through the drivers on the device — the "fsai" panel kind (two xk_csr_mm launches, no torch-expression
apply), cg / minres / bicgstab with the preconditioner, the `precond="fsai"` string forwards and backwards, batches,
and the iteration counts of a PCG loop written here.

The problem is the variable-coefficient grid operator at n = 24 (tests/fsai_cases.py, kappa ~ 6e3): in float64 plain CG
needs about 250 iterations at the drivers' default tolerance and CG with fsai(A) about 60, so the cap of 150 sits a
factor of about two from either side (tests/test_host_fsai.py runs the same on the host)."""
import warnings
import numpy as np
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import linop
from xitorch_amd.linop import LinearOperator, SparseLinearOperator
from xitorch_amd.linalg import solve, fsai, host_krylov
from xitorch_amd.linalg import precond as precond_mod
from xitorch_amd.linalg._panel import PanelOperator, pad_len
from tests import fsai_cases as fc

pytestmark = pytest.mark.gpu
n = 24
N = n * n
CAP = 150
F64, F32, C128 = torch.float64, torch.float32, torch.complex128


def _rhs(ncols=2, nb=None, dtype=F64, seed=5):
    shape = (N, ncols) if nb is None else (nb, N, ncols)
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if dtype.is_complex else 0)
    return torch.as_tensor(b).to(dtype)


def _boom(*a, **k):
    raise AssertionError("torch-expression apply on the device path")


def _no_torch_apply(monkeypatch):
    monkeypatch.setattr(linop, "csr_apply_torch", _boom)
    for cls in (linop.SparseLinearOperator, precond_mod.FSAIOperator):
        for name in ("_mm", "_mv", "_rmm", "_rmv"):
            monkeypatch.setattr(cls, name, _boom)


class _Generic(LinearOperator):
    """P applied as the torch expression G.rmm(G.mm(x)): the panel kind "generic" """

    def __init__(self, P):
        super().__init__(shape=P.shape, is_hermitian=True, dtype=P.dtype, device=P.device)
        self.P = P

    def _mv(self, x):
        return self._mm(x.unsqueeze(-1)).squeeze(-1)

    def _mm(self, x):
        return self.P.G.rmm(self.P.G.mm(x))

    def _getparamnames(self, prefix=""):
        return []


@pytest.mark.parametrize("dtype,phase", [(F64, False), (F32, False), (C128, True)])
def test_panel_kind_and_apply(dev, dtype, phase, monkeypatch):
    A, dense = fc.grid_operator(n, nmembers=3, dtype=dtype, device=dev, phase=phase)
    P = fsai(A)
    assert P.device.type == "cuda" and P.dtype == dtype and int(P.nfallback.sum()) == 0
    op = PanelOperator(P, [3], 3, N)
    gen = PanelOperator(_Generic(P), [3], 3, N)
    assert op.kind == "fsai" and gen.kind == "generic"
    assert op.pat._csc is not None, "the CSC view of G is built with the operator"
    Gd = torch.as_tensor(fc.g_dense(P))
    absP = Gd.abs().mH @ Gd.abs()
    eps = torch.finfo(dtype).eps
    g = torch.Generator().manual_seed(3)
    ld = pad_len(N)
    for p in (1, 3, 9, 3):
        X = torch.zeros((3, p, ld), dtype=dtype, device=dev)
        X[:, :, :N] = torch.randn(3, p, N, dtype=torch.float64, generator=g).to(dtype).to(dev)
        ref = gen.apply(X, torch.zeros_like(X))
        scr = op._scratch
        out = torch.full_like(X, 7.0)
        _no_torch_apply(monkeypatch)
        op.apply(X, out)
        monkeypatch.undo()
        assert op.last_kernel == "fsai"
        if scr is not None and scr.shape[1] >= p:
            assert op._scratch is scr, "the scratch panel is reallocated only when the column count grows"
        assert bool((out[:, :, N:] == 7.0).all()), "pads are not written"
        mag = (absP.to(torch.float64) @ X[:, :, :N].abs().cpu().to(torch.float64).transpose(-2, -1)).transpose(-2, -1)
        err = (out[:, :, :N] - ref[:, :, :N]).abs().cpu().to(torch.float64)
        assert bool((err <= 32 * eps * mag).all()), float((err / mag).max() / eps)
        # and against the dense product in double
        wide = torch.complex128 if dtype.is_complex else torch.float64
        dref = (Gd.to(wide).mH @ (Gd.to(wide) @ X[:, :, :N].cpu().to(wide).transpose(-2, -1))).transpose(-2, -1)
        assert bool(((out[:, :, :N].cpu().to(wide) - dref).abs() <= 32 * eps * mag).all())


def _resid_ok(dense, X, B, rtol):
    Ad = torch.as_tensor(dense).cpu()
    Ad = Ad.to(torch.complex128 if Ad.is_complex() else torch.float64)
    r = (Ad @ X.cpu().to(Ad.dtype) - B.cpu().to(Ad.dtype)).norm(dim=-2)
    return bool((r <= 2 * rtol * B.cpu().norm(dim=-2)).all())


@pytest.mark.parametrize("dtype,rtol", [(F64, 1e-6), (F32, 1e-4)])
@pytest.mark.parametrize("how", ["operator", "string"])
def test_cg_batch_of_three_within_the_cap(dev, dtype, rtol, how, monkeypatch):
    # three members with different conductances
    A, dense = fc.grid_operator(n, nmembers=3, dtype=dtype, device=dev)
    B = _rhs(nb=3, dtype=dtype).to(dev)
    before = dict(host_krylov.calls)
    pre = fsai(A) if how == "operator" else "fsai"
    _no_torch_apply(monkeypatch)
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(A, B, method="cg", max_niter=CAP, rtol=rtol, precond=pre, trace=tr)
    monkeypatch.undo()
    assert host_krylov.calls == before, "a device run reached a host driver"
    assert tr["converged"] and tr["niter"] <= CAP
    assert _resid_ok(A.fullmatrix(), X, B, rtol)          # (the operator as stored: fp32 rounds the conductances)
    if dtype == F64:
        with pytest.warns(xa.ConvergenceWarning):
            solve(A, B, method="cg", max_niter=CAP, rtol=rtol)


def test_minres_indefinite_complex_hermitian(dev):
    A, dense = fc.grid_operator(n, dtype=C128, device=dev, phase=True, batch=False)
    ev = np.linalg.eigvalsh(dense[0])
    shift = 0.5 * (ev[40] + ev[41])
    As, ds = fc.grid_operator(n, dtype=C128, device=dev, phase=True, batch=False, shift=shift)
    assert (np.linalg.eigvalsh(ds[0]) < 0).sum() == 41
    P = fsai(A)
    B = _rhs(dtype=C128).to(dev)
    before = dict(host_krylov.calls)
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(As, B, method="minres", precond=P, max_niter=4000, rtol=1e-8, trace=tr)
    assert host_krylov.calls == before and tr["converged"]
    assert _resid_ok(ds[0], X, B, 1e-7)


def test_bicgstab_with_left_preconditioner(dev):
    A, dense = fc.grid_operator(n, device=dev, batch=False)
    B = _rhs().to(dev)
    P = fsai(A)
    before = dict(host_krylov.calls)
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(A, B, method="bicgstab", precond_l=P)
        Xr = solve(A, B, method="bicgstab", precond_r=P, max_niter=CAP)
    assert host_krylov.calls == before
    assert _resid_ok(dense[0], X, B, 1e-6) and _resid_ok(dense[0], Xr, B, 1e-6)


def test_backward_with_the_string_equals_the_unpreconditioned_gradients(dev):
    m = 12
    crow, col, vals = fc.grid_csr(m)
    crow_d, col_d = torch.as_tensor(crow).to(dev), torch.as_tensor(col).to(dev)
    Bm = _rhs(seed=8)[:m * m].to(dev)
    opts = dict(method="cg", rtol=1e-12, atol=1e-14)
    grads = []
    for kw in (dict(precond="fsai"), dict()):
        v = torch.as_tensor(vals[0]).to(dev).requires_grad_()
        b = Bm.clone().requires_grad_()
        A = SparseLinearOperator(crow_d, col_d, v, (m * m, m * m), is_hermitian=True)
        x = solve(A, b, bck_options=dict(opts, **kw), **opts, **kw)
        grads.append(torch.autograd.grad((x ** 2).sum(), (v, b)))
    (gv1, gb1), (gv0, gb0) = grads
    assert torch.allclose(gv1, gv0, atol=1e-8, rtol=1e-6)
    assert torch.allclose(gb1, gb0, atol=1e-9, rtol=1e-7)


def _pcg_iterations(A, P, B, rtol=1e-8, cap=2000):
    """textbook preconditioned CG in float64 on A.mm / P.mm; -> iterations until every column has |r| <= rtol |b|"""
    x = torch.zeros_like(B)
    r = B.clone()
    z = P.mm(r) if P is not None else r
    p = z.clone()
    rz = (r * z).sum(-2, keepdim=True)
    stop = rtol * B.norm(dim=-2, keepdim=True)
    for k in range(1, cap + 1):
        Ap = A.mm(p)
        alpha = rz / (p * Ap).sum(-2, keepdim=True)
        x = x + alpha * p
        r = r - alpha * Ap
        if bool((r.norm(dim=-2, keepdim=True) <= stop).all()):
            return k
        z = P.mm(r) if P is not None else r
        rz_new = (r * z).sum(-2, keepdim=True)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return cap + 1


def test_iteration_counts(dev):
    A, dense = fc.grid_operator(n, device=dev, batch=False)
    B = _rhs(ncols=1).to(dev)
    plain = _pcg_iterations(A, None, B)
    p1 = _pcg_iterations(A, fsai(A, power=1), B)
    p2 = _pcg_iterations(A, fsai(A, power=2), B)
    print("pcg iterations at rtol 1e-8: plain %d, fsai(power=1) %d, fsai(power=2) %d" % (plain, p1, p2))
    assert 2 * p1 <= plain and p2 <= p1
