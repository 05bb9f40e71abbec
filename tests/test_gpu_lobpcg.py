"""-m gpu: `symeig(method="lobpcg")` on the HIP kernels — the cases of tests/test_host_lobpcg.py on the device (same
matrices, same assertions: tests/lobpcg_cases.py), and what the device path must respect: no host driver, no
torch-expression apply of a native operator, a native panel kernel, constant storage, a block that passes the guard.
The cap is 300 iterations as on the host; the device's iteration count is printed, not compared with the host's."""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import kernels as K
from xitorch_amd.linalg import symeig, svd, fsai, host_eig, _panel
from xitorch_amd.linalg.native_eig import GUARD_BAD
from xitorch_amd.linalg._panel import pad_len
from tests import chebfsi_cases as cc
from tests import lobpcg_cases as lc

pytestmark = pytest.mark.gpu
f64 = torch.float64


def run(op, neig, mode, dtype, M=None, **kw):
    tr = {}
    before = dict(host_eig.calls)
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        ev, X = symeig(op, neig, mode, M=M, method="lobpcg", min_eps=lc.min_eps(dtype), max_niter=lc.MAX_NITER,
                       trace=tr, **kw)
    assert dict(host_eig.calls) == before and ev.is_cuda and X.is_cuda
    assert tr["niter"] <= lc.MAX_NITER and tr["best_resid"] < lc.min_eps(dtype)
    print("device: niter %d napply %d best %.2e restarts %d redraws %d small_eigh %s kernel %s" % (
        tr["niter"], tr["napply"], tr["best_resid"], tr["restarts"], tr["redraws"], tr["small_eigh"],
        tr["panel_kernel"]))
    return ev, X, tr


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lc.IDS)
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
@pytest.mark.parametrize("neig", [1, 4, 6])
def test_dense(dev, dtype, mode, neig):
    A, lam = cc.dense_case(dtype, (), lc.N)
    ev, X, tr = run(xa.LinearOperator.m(A.to(dev), True), neig, mode, dtype)
    lc.assert_pairs(A, None, ev, X, neig, mode, dtype)
    assert tr["w"] == neig + max(2, -(-neig // 4)) and tr["small_eigh"] == "native"
    assert tr["panel_kernel"] in ("K1", "K1w", "K1wr", "K1s", "K1sw") and tr["torch_applies"] == 0


@pytest.mark.parametrize("batch", [(3,), (2, 2)], ids=["b3", "b2x2"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex64], ids=["f64", "c64"])
def test_batch_with_three_spectra(dev, batch, dtype):
    A, lam = cc.dense_case(dtype, batch, lc.N, spectrum=lc.batch_spectra(batch))
    ev, X, _ = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", dtype)
    assert ev.shape == (*batch, 4)
    lc.assert_pairs(A, None, ev, X, 4, "lowest", dtype)


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lc.IDS)
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_generalised(dev, dtype, mode):
    A, _ = cc.dense_case(dtype, (), 196)
    M = lc.overlap_matrix(14, dtype)
    ev, X, _ = run(xa.LinearOperator.m(A.to(dev), True), 4, mode, dtype, M=xa.LinearOperator.m(M.to(dev), True))
    lc.assert_pairs(A, M, ev, X, 4, mode, dtype)


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lc.IDS)
@pytest.mark.parametrize("precond", ["none", "diag", "tensor"])
def test_diagonally_dominant(dev, dtype, precond):
    A = lc.dominant_matrix(dtype)
    pc = {"none": None, "diag": "diag", "tensor": torch.diagonal(A).real.clone().to(dev)}[precond]
    ev, X, tr = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", dtype, precond=pc)
    lc.assert_pairs(A, None, ev, X, 4, "lowest", dtype)
    if precond != "none" and lc.REAL_OF[dtype] == f64:
        assert tr["niter"] < 40


def test_generalised_with_diagonal_preconditioner(dev):
    A = lc.dominant_matrix(f64, n=196)
    M = lc.overlap_matrix(14, f64)
    ev, X, _ = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", f64, M=xa.LinearOperator.m(M.to(dev), True),
                   precond="diag")
    lc.assert_pairs(A, M, ev, X, 4, "lowest", f64)


@pytest.mark.parametrize("kind,precond", [("sparse", False), ("sparse", True), ("banded", False), ("mv", False)],
                         ids=["csr", "csr-fsai", "banded", "mv"])
def test_grid_with_double_eigenvalues(dev, kind, precond):
    A = lc.grid_matrix(16)
    op = lc.operator_of(kind, A, dev)
    ev, X, tr = run(op, 6, "lowest", f64, precond=fsai(op) if precond else None)
    lc.assert_pairs(A, None, ev, X, 6, "lowest", f64)
    if kind == "mv":
        assert tr["panel_kernel"] == "generic" and tr["torch_applies"] == tr["napply"]
    else:
        # a device operator of a native storage kind never reaches a torch-expression apply
        assert tr["panel_kernel"] == {"sparse": "csr", "banded": "banded"}[kind] and tr["torch_applies"] == 0


def test_v0_with_three_exact_eigenvectors_of_four(dev):
    A, lam, Q = cc.dense_case(f64, (), lc.N, with_vectors=True)
    ev, X, tr = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", f64, V0=Q[:, :3].to(dev))
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)


def test_exact_v0_converges_in_zero_iterations(dev):
    A, lam, Q = cc.dense_case(f64, (), lc.N, with_vectors=True)
    ev, X, tr = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", f64, V0=Q[:, :6].to(dev))
    assert tr["niter"] == 0 and tr["napply"] == 1
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)


def test_diagonal_operator_and_cluster(dev):
    A = torch.diag(torch.arange(1, lc.N + 1, dtype=f64))
    for pc in (None, "diag"):
        ev, X, _ = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", f64, precond=pc)
        lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)
    A, lam = cc.dense_case(f64, (), lc.N, spectrum=lc.cluster_spectrum())
    ev, X, _ = run(xa.LinearOperator.m(A.to(dev), True), 6, "lowest", f64)
    lc.assert_pairs(A, None, ev, X, 6, "lowest", f64)


def test_two_iterations_warn_and_return_the_best_block(dev):
    A, lam = cc.dense_case(f64, (), lc.N)
    tr = {}
    with pytest.warns(xa.ConvergenceWarning):
        ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", method="lobpcg", min_eps=1e-10, max_niter=2,
                       trace=tr)
    assert tr["niter"] == 2 and tr["best_resid"] >= 1e-10
    ev, X = ev.cpu(), X.cpu()
    assert bool(torch.isfinite(ev).all()) and bool(torch.isfinite(X).all())
    R = A @ X - X * ev.unsqueeze(-2)
    assert abs(float(R.abs().max()) - tr["best_resid"]) <= 1e-11
    assert float((X.T @ X - torch.eye(4, dtype=f64)).abs().max()) <= GUARD_BAD[f64]


def test_device_operators_never_reach_the_host_twin(dev, monkeypatch):
    """asserted the way tests/test_gpu_davidson.py::test_device_operators_never_reach_the_host_drivers does"""
    from xitorch_amd import _capi
    A, lam = cc.dense_case(f64, (), lc.N)
    Ad = xa.LinearOperator.m(A.to(dev), True)
    before = dict(host_eig.calls)
    tr = {}
    symeig(Ad, 3, "lowest", method="lobpcg", min_eps=1e-8, max_niter=lc.MAX_NITER, trace=tr)
    assert dict(host_eig.calls) == before and tr["torch_applies"] == 0
    with pytest.raises(_capi.NativeLibraryError):
        host_eig.lobpcg(Ad, 3, "lowest")
    n_host = host_eig.calls["lobpcg"]
    symeig(xa.LinearOperator.m(A, True), 3, "lowest", method="lobpcg", min_eps=1e-8, max_niter=lc.MAX_NITER)
    assert host_eig.calls["lobpcg"] == n_host + 1

    def gone(*a, **k):
        raise _capi.NativeLibraryError("libxitorch_amd.so not found (simulated)")
    monkeypatch.setattr(_capi, "fn", gone)
    monkeypatch.setattr(K, "fn", gone)
    monkeypatch.setattr(_panel, "fn", gone)
    with pytest.raises(_capi.NativeLibraryError):
        symeig(Ad, 3, "lowest", method="lobpcg", min_eps=1e-8)


def test_refusals_and_handover_on_the_device(dev):
    A, _ = cc.dense_case(f64, (), lc.N)
    op = xa.LinearOperator.m(A.to(dev), True)
    with pytest.raises(NotImplementedError):
        symeig(op, 3, "lowest", method="lobpcg", process_group=object())
    with pytest.raises(NotImplementedError, match="chebfsi"):
        symeig(op, 30, "lowest", method="lobpcg")
    with pytest.raises(RuntimeError, match="Unknown lobpcg preconditioner"):
        symeig(op, 3, "lowest", method="lobpcg", precond="davidson")
    A24, lam24 = cc.dense_case(f64, (), 24)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A24.to(dev), True), 4, "lowest", method="lobpcg", trace=tr)
    assert tr["handed_to"] == "exacteig" and float((ev.cpu() - lam24[:4]).abs().max()) < 1e-10


def test_storage_does_not_grow_with_the_iteration_count(dev):
    """N = 4099, w = 8, a generalised problem with an operator preconditioner (every buffer the driver can have).
    Panel buffers, from the code of native_lobpcg.lobpcg: the three stacks (9 w rows) and c = 3 panels of w rows —
    the best block, the spare random directions, the preconditioner's output; the start block is released before the
    first iteration.  Next to them lives one more panel at a time that is not the driver's: the start block until the
    first iteration, FSAI's own scratch panel (inside the preconditioner operator) from then on; and one panel is
    allowed for a transient of a single torch expression or kernel wrapper (the driver's own passes over a panel are
    in place).  So c = 3 + 1 + 1 panels of w rows: 14 w rows in all, where a second copy of the stacks would need
    21 w.  The small matrices — a dozen of order 3 w = 24 at most (Gram blocks, T_S, its eigenvectors, C and the QR
    of C_p: 12 x 24 x 24 x 8 B = 55 KB), the partial sums and status words — get 64 KiB.  Nothing in that depends on
    niter: a run of 3 and a run of 30 iterations must peak within the same bound, and within 64 KiB of each other."""
    n, w, neig = 4099, 8, 6
    d = 2.0 + torch.arange(n, dtype=f64) * 1e-3
    off = -0.5 * torch.ones(n - 1, dtype=f64)
    A = torch.diag(d) + torch.diag(off, 1) + torch.diag(off, -1)
    Mm = torch.eye(n, dtype=f64) + 0.1 * (torch.diag(torch.ones(n - 1, dtype=f64), 1) +
                                          torch.diag(torch.ones(n - 1, dtype=f64), -1))
    op, Mop = lc.csr_of(A, dev), lc.csr_of(Mm, dev)
    pc = fsai(op)
    peaks = []
    for niter in (1, 3, 30):                                         # (the first run fills the cached workspaces)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tr = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", xa.ConvergenceWarning)
            ev, X = symeig(op, neig, "lowest", M=Mop, method="lobpcg", nguard=w - neig, precond=pc, min_eps=1e-30,
                           max_niter=niter, trace=tr)
        torch.cuda.synchronize()
        if niter > 1:
            peaks.append(torch.cuda.max_memory_allocated() - base)
        assert tr["niter"] == niter and tr["w"] == w
        assert tr["panel_buffers"] == 9 + 3                          # in units of (Bt, w, ld): the stacks and c = 3
        assert tr["panel_kernel"] == "csr" and tr["torch_applies"] == 0
        del ev, X
    c = 3 + 1 + 1
    bound = (9 * w + c * w) * pad_len(n) * 1 * 8 + (64 << 10)
    print("peak growth over the call: %d and %d bytes, bound %d" % (peaks[0], peaks[1], bound))
    assert max(peaks) <= bound and abs(peaks[1] - peaks[0]) <= (64 << 10)


def test_dependent_start_vectors_recover(dev):
    """V0 with two identical columns: the run recovers and returns a block that passes the guard"""
    A, lam = cc.dense_case(f64, (), lc.N)
    V0 = torch.randn(lc.N, 6, dtype=f64, generator=torch.Generator().manual_seed(2))
    V0[:, 3] = V0[:, 1]
    ev, X, tr = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", f64, V0=V0.to(dev))
    assert tr["redraws"] + tr["restarts"] > 0
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)


def test_cholesky_flag_of_the_new_directions_discards_the_iterate(dev, monkeypatch):
    """The flag of W's CholeskyQR reaches the host with the iteration's status read, after the rotation: that iterate is
    never kept, the run restarts from the best block without P and still converges.  Forced here by raising the flag
    after the second orthonormalisation call (the first is the start block's)."""
    A, lam = cc.dense_case(f64, (), lc.N)
    real_orth, ncall = K.davidson_orth, [0]

    def flagged(V, N, k0, q, C, W, info, passes=2, cond=None):
        real_orth(V, N, k0, q, C, W, info, passes=passes, cond=cond)
        ncall[0] += 1
        if ncall[0] == 2:
            info.fill_(3)
    monkeypatch.setattr(K, "davidson_orth", flagged)
    ev, X, tr = run(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", f64)
    assert ncall[0] > 2 and tr["restarts"] == 1 and tr["redraws"] == 0
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)


def test_backward_and_svd(dev):
    g = torch.Generator().manual_seed(7)
    A0, _ = cc.dense_case(f64, (), 40)
    W = torch.randn(40, 3, dtype=f64, generator=g).to(dev)
    grads = {}
    for meth, kw in (("lobpcg", dict(min_eps=1e-10, max_niter=lc.MAX_NITER)), ("exacteig", {})):
        Ap = A0.clone().to(dev).requires_grad_()
        ev, X = symeig(xa.LinearOperator.m(Ap, True), 3, "lowest", method=meth, **kw)
        loss = (ev * torch.arange(1, 4, dtype=f64, device=dev)).sum() + ((X * W).sum(0) ** 2).sum()
        grads[meth], = torch.autograd.grad(loss, Ap)
    ga, gb = grads["lobpcg"], grads["exacteig"]
    ga, gb = (ga + ga.T) * 0.5, (gb + gb.T) * 0.5
    assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max())
    B = torch.randn(60, 40, dtype=f64, generator=torch.Generator().manual_seed(11))
    u, s, vh = svd(xa.LinearOperator.m(B.to(dev)), 3, method="lobpcg", min_eps=1e-10, max_niter=lc.MAX_NITER)
    want = torch.linalg.svdvals(B)[:3]
    assert float((s.cpu().sort(descending=True)[0] - want).abs().max()) <= 1e-8 * float(want[0])
