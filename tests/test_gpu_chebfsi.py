"""-m gpu: `symeig(method="chebfsi")` on the HIP kernels — the cases of tests/test_host_chebfsi.py on the device (same
matrices, same assertions: tests/chebfsi_cases.py), agreement with the host twin, and what the device path must not
touch: torch.linalg.eigh inside the native widths, torch-expression applies, the host drivers.

`trace["small_eigh"] == "native"` is asserted for every block of w <= EXACTEIG_NATIVE_MAX_P vectors in the dense
known-spectrum cases, all four dtypes."""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import kernels as K
from xitorch_amd.linalg import symeig, host_eig, native_chebfsi, _panel
from xitorch_amd.linalg.native_eig import EXACTEIG_NATIVE_MAX_P
from tests import chebfsi_cases as cc

pytestmark = pytest.mark.gpu
DTYPES, IDS = cc.DTYPES, cc.IDS


@pytest.fixture(autouse=True)
def _no_convergence_warnings():
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        yield


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("neig", [1, 6, 24])
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_known_spectrum_dense_and_agreement_with_the_host_twin(dev, dtype, neig, mode):
    A, lam = cc.dense_case(dtype, (), cc.N)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), neig, mode, method="chebfsi", min_eps=cc.min_eps(dtype),
                   trace=tr)
    assert ev.is_cuda and X.is_cuda
    cc.assert_pairs(A, lam, ev, X, neig, mode, dtype)
    w = neig + max(8, -(-neig // 4))
    assert tr["w"] == w and tr["guard_redo"] == []
    assert w <= EXACTEIG_NATIVE_MAX_P and tr["small_eigh"] == "native"
    ev_h, X_h = symeig(xa.LinearOperator.m(A, True), neig, mode, method="chebfsi", min_eps=cc.min_eps(dtype))
    cc.assert_pairs(A, lam, ev_h, X_h, neig, mode, dtype)
    bound = cc.eigenvalue_bound(cc.N, cc.min_eps(dtype), dtype, float(lam.abs().max()))
    assert float((ev.cpu().double() - ev_h.double()).abs().max()) <= bound


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_2x3_with_a_broadcast_dimension(dev, dtype):
    A, lam = cc.dense_case(dtype, (2, 1), cc.N)
    Ab = A.expand(2, 3, cc.N, cc.N)
    ev, X = symeig(xa.LinearOperator.m(Ab.to(dev).contiguous(), True), 6, "lowest", method="chebfsi",
                   min_eps=cc.min_eps(dtype))
    assert ev.shape == (2, 3, 6) and X.shape == (2, 3, cc.N, 6)
    cc.assert_pairs(Ab, lam.expand(2, 3, cc.N), ev, X, 6, "lowest", dtype)


KIND_CASES = [(k, d) for k in ("banded", "sparse", "mv") for d in DTYPES if not (k == "banded" and d.is_complex)]


@pytest.mark.parametrize("kind,dtype", KIND_CASES, ids=["%s-%s" % (k, IDS[DTYPES.index(d)]) for k, d in KIND_CASES])
def test_operator_kinds(dev, kind, dtype):
    op, A, lam = cc.operator_case(kind, dtype, dev)
    tr = {}
    ev, X = symeig(op, 6, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype), trace=tr)
    cc.assert_pairs(A, lam, ev, X, 6, "lowest", dtype)
    assert tr["panel_kernel"] == {"banded": "banded", "sparse": "csr", "mv": "generic"}[kind]


@pytest.mark.parametrize("n,kernel", [(1024, "K1w"), (1030, "K1")])
def test_wide_block_on_symmetric_fp32_storage(dev, n, kernel):
    """neig = 24 (w = 32 columns) on exactly symmetric fp32 storage.  Order 1024: the matrix-core wide form K1w serves
    every apply of the filter.  Order 1030 is no multiple of the 128-column tile of K1w (DESIGN section 3.0:
    `kernels._wide_ok`), so the dispatch takes the VALU form K1 there: asserted as such."""
    A, lam = cc.dense_case(torch.float32, (), n, seed=1)
    op = xa.LinearOperator.m(A.to(dev), True)
    assert op.symmetric_storage
    eps_ = cc.MIN_EPS32_1K                        # 4 x the host twin's measured floor at these orders
    tr = {}
    ev, X = symeig(op, 24, "lowest", method="chebfsi", min_eps=eps_, trace=tr)
    cc.assert_pairs(A, lam, ev, X, 24, "lowest", torch.float32, eps_=eps_)
    assert tr["w"] == 32 and tr["panel_kernel"] == kernel and tr["small_eigh"] == "native"


def test_no_library_eigh_and_no_torch_apply_on_the_device_path(dev, monkeypatch):
    """real blocks inside the native widths: torch.linalg.eigh is never called; a device CSR operator and a complex
    Hermitian dense operator are applied by the HIP kernels only (their torch expressions are patched to raise)"""
    from xitorch_amd import linop

    def boom(*a, **k):
        raise AssertionError("library eigh / torch-expression apply on the device path")
    A, lam = cc.dense_case(torch.float64, (), cc.N)
    opc, Ac, lamc = cc.operator_case("sparse", torch.complex128, dev)
    Ah, lamh = cc.dense_case(torch.complex128, (), cc.N)
    oph = xa.LinearOperator.m(Ah.to(dev), True)
    opd = xa.LinearOperator.m(A.to(dev), True)
    monkeypatch.setattr(linop, "csr_apply_torch", boom)
    monkeypatch.setattr(linop.MatrixLinearOperator, "_mm", boom)
    monkeypatch.setattr(linop.MatrixLinearOperator, "_mv", boom)
    monkeypatch.setattr(linop.SparseLinearOperator, "_mm", boom)
    monkeypatch.setattr(linop.SparseLinearOperator, "_mv", boom)
    monkeypatch.setattr(torch.linalg, "eigh", boom)
    trc, trh, tr = {}, {}, {}
    ev_c, X_c = native_chebfsi.chebfsi(opc, 4, "lowest", min_eps=1e-8, trace=trc)          # w = 12
    ev_h, X_h = native_chebfsi.chebfsi(oph, 24, "uppest", min_eps=1e-8, trace=trh)         # w = 32
    ev, X = native_chebfsi.chebfsi(opd, 24, "lowest", min_eps=1e-8, trace=tr)
    assert tr["small_eigh"] == trc["small_eigh"] == trh["small_eigh"] == "native"
    monkeypatch.undo()
    cc.assert_pairs(A, lam, ev, X, 24, "lowest", torch.float64)
    cc.assert_pairs(Ac, lamc, ev_c, X_c, 4, "lowest", torch.complex128)
    cc.assert_pairs(Ah, lamh, ev_h, X_h, 24, "uppest", torch.complex128)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["f64", "c128"])
def test_clustered_pair_inside_the_block(dev, dtype):
    """two wanted eigenvalues 1e-3 apart: residual and orthonormality only"""
    spec = torch.arange(cc.N, dtype=torch.float64)
    spec[3] = spec[2] + 1e-3
    A, lam = cc.dense_case(dtype, (), cc.N, spectrum=spec)
    ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 6, "lowest", method="chebfsi", min_eps=1e-8)
    cc.assert_residual_and_orthonormality(A, ev, X, 1e-8, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_operator(dev, dtype):
    """Lanczos with beta = 0, the identity filter of an interval without width, CholeskyQR of an unfiltered block"""
    A = torch.zeros(cc.N, cc.N, dtype=dtype)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 4, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype),
                   trace=tr)
    # eigenvalues by the bound of every other case, |lam_hat - 0| <= sqrt(N) min_eps + 64 eps |A|_2 with |A|_2 = 0 (the
    # native dense eigensolver locates eigenvalues by bisection down to the smallest normal number, not to exact zero)
    assert float(ev.abs().max()) <= cc.eigenvalue_bound(cc.N, cc.min_eps(dtype), dtype, 0.0) and tr["guard_redo"] == []
    cc.assert_residual_and_orthonormality(A, ev, X, cc.min_eps(dtype), dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex64], ids=["f64", "c64"])
def test_start_block_is_honoured(dev, dtype):
    """the exact invariant subspace as V0: converged at the first Rayleigh-Ritz; narrower / wider V0"""
    A, lam, Q = cc.dense_case(dtype, (), cc.N, with_vectors=True)
    op = xa.LinearOperator.m(A.to(dev), True)
    eps_ = cc.min_eps(dtype)
    tr = {}
    ev, X = symeig(op, 6, "lowest", method="chebfsi", min_eps=eps_, V0=Q[:, :14].to(dev), trace=tr)
    assert tr["niter"] == 1 and tr["w"] == 14
    cc.assert_pairs(A, lam, ev, X, 6, "lowest", dtype)
    tr = {}
    ev, X = symeig(op, 6, "lowest", method="chebfsi", min_eps=eps_, V0=Q[:, :3], trace=tr)       # (a host V0 is moved)
    assert tr["w"] == 14
    cc.assert_pairs(A, lam, ev, X, 6, "lowest", dtype)
    tr = {}
    symeig(op, 6, "lowest", method="chebfsi", min_eps=eps_, V0=Q[:, :20].to(dev), trace=tr)
    assert tr["w"] == 20 and tr["niter"] == 1


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["f64", "c128"])
def test_one_iteration_on_a_hard_spectrum_warns_and_returns_the_best_block(dev, dtype):
    from xitorch_amd.linalg.native_eig import GUARD_BAD
    spec = 1.0 + torch.arange(cc.N, dtype=torch.float64) * 1e-3          # relative gaps of 1e-3
    A, lam = cc.dense_case(dtype, (), cc.N, spectrum=spec)
    tr = {}
    with pytest.warns(xa.ConvergenceWarning):
        ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 6, "lowest", method="chebfsi", min_eps=1e-10, max_niter=1,
                       trace=tr)
    assert tr["niter"] == 1 and tr["best_resid"] >= 1e-10
    Aw, Xw = A.to(torch.complex128), X.cpu().to(torch.complex128)
    R = Aw @ Xw - Xw * ev.cpu().to(torch.complex128).unsqueeze(-2)
    # the returned block IS the one whose residual was recorded (recomputed in 128-bit complex: rounding of A X only)
    assert abs(float(R.abs().max()) - tr["best_resid"]) <= 1e-11
    G = Xw.transpose(-2, -1).conj() @ Xw - torch.eye(6, dtype=torch.complex128)
    assert float(G.abs().max()) <= GUARD_BAD[torch.float64]


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64], ids=["c128", "c64"])
def test_complex_block_wider_than_one_cholqr_chunk(dev, dtype):
    """neig = 40 (w = 50): the complex block is orthonormalised in chunks of 32 vectors"""
    A, lam = cc.dense_case(dtype, (), cc.N)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 40, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype),
                   trace=tr)
    assert tr["w"] == 50 and tr["guard_redo"] == []
    # complex blocks wider than 32 vectors: the Rayleigh-Ritz matrix goes to the library eigh
    assert tr["small_eigh"] == "library"
    cc.assert_pairs(A, lam, ev, X, 40, "lowest", dtype)


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64], ids=["c128", "c64"])
def test_degenerate_pair_at_the_seam_of_the_two_eigensolver_calls(dev, dtype):
    """neig = 12 (w = 20): the block's Rayleigh-Ritz takes two xk_herm_eigh calls, pairs 1 .. 16 and 17 .. 20.  The
    spectrum has an exactly degenerate pair at positions 16 / 17 of the block (lam_15 = lam_16, counted from 0): vectors
    of separate calls are not orthogonal to each other there, the driver must notice (that call
    goes to the library) — no guard redo, no error, all wanted pairs by order."""
    spec = torch.arange(cc.N, dtype=torch.float64)
    spec[16] = spec[15]
    A, lam = cc.dense_case(dtype, (), cc.N, spectrum=spec)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 12, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype),
                   trace=tr)
    assert tr["w"] == 20 and tr["guard_redo"] == [] and tr["small_eigh"] == "library"
    cc.assert_pairs(A, lam, ev, X, 12, "lowest", dtype)
    # and with the pair merely close (gap 1e-4 of the block's |T|: below the c64 threshold 2.4e-3, above the c128 one
    # 2.2e-6, where the two native sets are joined by the projection)
    spec[16] = spec[15] + 2e-3
    A, lam = cc.dense_case(dtype, (), cc.N, spectrum=spec)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 12, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype),
                   trace=tr)
    assert tr["guard_redo"] == []
    cc.assert_pairs(A, lam, ev, X, 12, "lowest", dtype)


def test_device_operators_never_reach_the_host_twin(dev, monkeypatch):
    from xitorch_amd import _capi
    A, lam = cc.dense_case(torch.float64, (), cc.N)
    Ad = xa.LinearOperator.m(A.to(dev), True)
    before = dict(host_eig.calls)
    symeig(Ad, 3, "lowest", method="chebfsi", min_eps=1e-8)
    assert dict(host_eig.calls) == before
    with pytest.raises(_capi.NativeLibraryError):
        host_eig.chebfsi(Ad, 3, "lowest")
    n_host = host_eig.calls["chebfsi"]
    symeig(xa.LinearOperator.m(A, True), 3, "lowest", method="chebfsi", min_eps=1e-8)
    assert host_eig.calls["chebfsi"] == n_host + 1

    def gone(*a, **k):
        raise _capi.NativeLibraryError("libxitorch_amd.so not found (simulated)")
    monkeypatch.setattr(_capi, "fn", gone)
    monkeypatch.setattr(K, "fn", gone)
    monkeypatch.setattr(_panel, "fn", gone)          # (the drivers' one direct use of fn: kry_blocks)
    with pytest.raises(_capi.NativeLibraryError):
        symeig(Ad, 3, "lowest", method="chebfsi", min_eps=1e-8)


def test_refusals_and_handover_on_the_device(dev):
    A, _ = cc.dense_case(torch.float64, (), cc.N)
    op = xa.LinearOperator.m(A.to(dev), True)
    Mop = xa.LinearOperator.m(torch.eye(cc.N, dtype=torch.float64, device=dev), True)
    with pytest.raises(NotImplementedError, match="davidson"):
        symeig(op, 3, "lowest", M=Mop, method="chebfsi")
    with pytest.raises(NotImplementedError, match="davidson"):
        symeig(op, 3, "lowest", method="chebfsi", process_group=object())
    A40, lam40 = cc.dense_case(torch.float64, (), 40)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A40.to(dev), True), 32, "lowest", method="chebfsi", trace=tr)
    assert tr["handed_to"] == "exacteig"
    cc.assert_pairs(A40, lam40, ev, X, 32, "lowest", torch.float64)


def test_larger_closed_form_spectrum_fp64(dev):
    """2 x 4096 dense fp64, neig = 32 (w = 40): residual, orthonormality, eigenvalues.  A = H D H with a Householder
    reflector H = I - 2 v v^T: the spectrum is D exactly and the matrix costs O(n^2) to build."""
    n = 4096
    spec = torch.cat((torch.arange(48, dtype=torch.float64), 48.0 + torch.arange(n - 48, dtype=torch.float64) * 0.05))
    g = torch.Generator().manual_seed(5)
    v = torch.randn(2, n, 1, dtype=torch.float64, generator=g)
    v = v / torch.linalg.vector_norm(v, dim=-2, keepdim=True)
    D = spec.expand(2, n)
    Dv = D.unsqueeze(-1) * v
    A = torch.diag_embed(D) - 2.0 * v @ Dv.transpose(-2, -1) - 2.0 * Dv @ v.transpose(-2, -1) \
        + 4.0 * (v.transpose(-2, -1) @ Dv) * (v @ v.transpose(-2, -1))
    A = (A + A.transpose(-2, -1)) * 0.5
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A.to(dev), True), 32, "lowest", method="chebfsi", min_eps=1e-8, trace=tr)
    cc.assert_pairs(A, D, ev, X, 32, "lowest", torch.float64)
    assert tr["w"] == 40 and tr["small_eigh"] == "native"


def test_backward_matches_exacteig_on_the_device(dev):
    g = torch.Generator().manual_seed(7)
    A0, _ = cc.dense_case(torch.float64, (), 40)
    W = torch.randn(40, 3, dtype=torch.float64, generator=g).to(dev)
    grads = {}
    for meth, kw in (("chebfsi", dict(min_eps=1e-10)), ("exacteig", {})):
        Ap = A0.to(dev).clone().requires_grad_()
        ev, X = symeig(xa.LinearOperator.m(Ap, True), 3, "lowest", method=meth, **kw)
        loss = (ev * torch.arange(1, 4, dtype=torch.float64, device=dev)).sum() + ((X * W).sum(0) ** 2).sum()
        grads[meth], = torch.autograd.grad(loss, Ap)
    ga, gb = grads["chebfsi"], grads["exacteig"]
    ga, gb = (ga + ga.T) * 0.5, (gb + gb.T) * 0.5
    assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max())
