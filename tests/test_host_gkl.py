"""CPU: svd(method="gkl") on operators in host memory (host_eig.gkl, the torch-op twin of native_gkl.gkl), checked by
the a-posteriori bounds of tests/gkl_cases.py: |s - sigma| <= sqrt(2) r (Weyl on the augmented operator), r <= 2 min_eps
sigma_max, orthonormality within ORTH_C u ncv; min_eps = 100 u throughout."""
import warnings
import numpy as np
import pytest
import torch
from tests import gkl_cases as gc
from xitorch_amd import LinearOperator
from xitorch_amd.linalg import svd
from xitorch_amd.linalg import host_eig


def _run(A, k, mode, ncv=None, op=None, **opts):
    min_eps = 100 * gc.unit_roundoff(A.dtype)
    trace = {}
    before = host_eig.calls["gkl"]
    op = LinearOperator.m(A) if op is None else op
    with torch.no_grad():
        u, s, vh = svd(op, k=k, mode=mode, method="gkl", min_eps=min_eps, ncv=ncv, trace=trace, **opts)
    assert host_eig.calls["gkl"] == before + 1 and trace["converged"]
    assert u.shape == (*A.shape[:-2], A.shape[-2], k) and vh.shape == (*A.shape[:-2], k, A.shape[-1])
    err, r = gc.check(A, u, s, vh, k, mode, min_eps, trace["ncv"],
                      label="%s %s %s" % (tuple(A.shape), A.dtype, mode))
    return trace, (u, s, vh), (err, r)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(300, 200), (200, 300), (257, 257)])
def test_graded_spectrum_and_the_squared_route(dtype, shape):
    A = gc.graded(*shape).to(dtype)
    k = 10
    trace, _, (err, r) = _run(A, k, "uppest")
    # the reason the feature exists: the A^H A route loses every value below sqrt(u) sigma_max
    ur = gc.unit_roundoff(dtype)
    sig = gc.true_values(A, k, "uppest")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, s_sq, _ = svd(LinearOperator.m(A), k=k, mode="uppest", method="davidson", min_eps=1e-3 * ur, max_niter=60)
    small = sig < np.sqrt(ur) * sig.max()
    assert small.sum() >= 2
    miss = np.abs(s_sq.double().numpy() - sig) > 2.0 ** 0.5 * r
    print("squared route: |s - sigma| / u sigma_max =", np.abs(s_sq.double().numpy() - sig) / (ur * sig.max()))
    assert miss[small].all()


@pytest.mark.parametrize("shape", [(400, 260), (260, 400)])
def test_slow_spectrum_needs_restarts(shape):
    trace, _, _ = _run(gc.slow(*shape), 6, "uppest", ncv=14)
    assert trace["restarts"] >= 2 and trace["keep"] == 6 + (14 - 6) // 2


@pytest.mark.parametrize("shape", [(120, 80), (80, 120), (96, 96)])
def test_lowest_in_both_orientations(shape):
    trace, (_, s, _), _ = _run(gc.lowest(*shape), 3, "lowest")
    assert trace["tall"] == (shape[0] >= shape[1])
    assert np.allclose(s.numpy(), [1e-3, 2e-3, 4e-3], rtol=1e-9, atol=0)      # ascending, the planted values
    assert trace["niter"] <= 30


def test_batch_of_three_converging_unevenly():
    trace, _, _ = _run(gc.uneven_batch(), 4, "uppest", ncv=12)
    gc.check_uneven(trace, 4)                                  # member 0 is done while the slow member needs restarts
    assert len(trace["resid_history"]) == trace["niter"]


def test_complex128():
    for shape in ((150, 100), (100, 150)):
        _run(gc.graded(*shape, cplx=True), 8, "uppest")
    _run(gc.lowest(80, 120, cplx=True), 3, "lowest")


def test_v0_start():
    A = gc.slow(400, 260)
    V0 = torch.linalg.svd(A)[2][:6].transpose(0, 1).contiguous()
    cold, _, _ = _run(A, 6, "uppest", ncv=14)
    warm, _, _ = _run(A, 6, "uppest", ncv=14, V0=V0)
    assert warm["niter"] <= cold["niter"]
    At = gc.slow(260, 400)
    _run(At, 6, "uppest", ncv=14, V0=torch.linalg.svd(At)[2][:6].transpose(0, 1).contiguous())


def test_rank_deficient_and_exact_breakdown():
    _run(gc.rank_deficient(120, 90, 12), 5, "uppest")
    d = np.linspace(1.0, 0.05, 90) ** 2
    A = torch.zeros((120, 90), dtype=torch.float64)
    A[torch.arange(90), torch.arange(90)] = torch.from_numpy(d)
    V0 = torch.zeros((90, 1), dtype=torch.float64)
    V0[0, 0] = 1.0
    trace, _, _ = _run(A, 5, "uppest", V0=V0)
    assert trace["breakdowns"] and trace["breakdowns"][0][0] == 1               # the first beta is exactly zero


def test_small_problem_goes_to_the_dense_svd():
    A = gc.with_spectrum(30, 14, np.linspace(1.0, 0.1, 14), seed=9)
    trace = {}
    u, s, vh = svd(LinearOperator.m(A), k=3, mode="lowest", method="gkl", trace=trace)
    assert trace["handed_to"] == "dense_svd"
    assert np.allclose(s.numpy(), gc.true_values(A, 3, "lowest"), rtol=1e-12)
    assert gc.residual(A, u, s, vh) <= 1e-13


def test_refusals_and_warning():
    op = LinearOperator.m(gc.graded(300, 200))
    with pytest.raises(NotImplementedError):
        svd(op, k=4, method="gkl", process_group=object())
    with pytest.raises(ValueError):
        svd(op, k=4, method="gkl", ncv=65)
    with pytest.raises(ValueError):
        svd(op, k=20, method="gkl", ncv=20)
    with pytest.raises(ValueError):
        svd(op, k=30, method="gkl")                                             # default ncv = 68 > 64
    with pytest.warns(Warning, match="convergence is not achieved"):
        svd(LinearOperator.m(gc.slow(400, 260)), k=6, method="gkl", ncv=14, max_niter=1, min_eps=1e-14)


def test_other_methods_keep_their_route_bit_for_bit():
    A = gc.with_spectrum(60, 40, np.linspace(1.0, 0.1, 40), seed=4)
    op = LinearOperator.m(A)
    AA = op.H.matmul(op, is_hermitian=True)
    from xitorch_amd.linalg import symeig
    for method in (None, "davidson"):
        u, s, vh = svd(op, k=3, mode="uppest", method=method)
        ev, evec = symeig(AA, 3, "uppest", method=method)
        assert torch.equal(s, torch.sqrt(torch.clamp(ev, min=0.0))) and torch.equal(vh, evec.transpose(-2, -1).conj())


def _loss(u, s, vh, w):
    # gauge-invariant: sum of the values, a weighted rank-k reconstruction norm, one entry of u_k v_k^H
    rec = (u * w) @ vh
    return s.sum() + (rec.abs() ** 2).sum().sqrt() + (u[..., :, -1:] @ vh[..., -1:, :])[..., 0, 1].real.sum()


@pytest.mark.parametrize("shape", [(12, 9), (9, 12)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_gradient(shape, cplx):
    """gradcheck of the implicit backward on the augmented operator, and agreement with torch.linalg.svd's autograd.
    (order 9 <= 16: the forward is the dense hand-off, the backward is the one every gkl call uses)"""
    s = np.linspace(2.0, 0.4, 9)
    A0 = gc.with_spectrum(*shape, s, seed=21, cplx=cplx)
    w = torch.linspace(1.0, 2.0, 3, dtype=torch.float64)
    bck = {"method": "minres", "rtol": 1e-13, "atol": 1e-15, "max_niter": 200}

    def f(A):
        u, sv, vh = svd(LinearOperator.m(A), k=3, mode="uppest", method="gkl", bck_options=bck)
        return _loss(u, sv, vh, w)

    A = A0.clone().requires_grad_()
    assert torch.autograd.gradcheck(f, (A,), eps=1e-6, atol=1e-6, rtol=1e-5)
    f(A).backward()
    Ar = A0.clone().requires_grad_()
    U, S, Vh = torch.linalg.svd(Ar, full_matrices=False)
    idx = torch.tensor([2, 1, 0])
    _loss(U[:, idx], S[idx], Vh[idx], w).backward()
    assert (A.grad - Ar.grad).abs().max() <= 1e-9 * Ar.grad.abs().max()


def test_gradient_through_the_iteration():
    """the same backward behind the Lanczos forward (short side 24 > 16), against the dense autograd"""
    A0 = gc.with_spectrum(40, 24, np.linspace(2.0, 0.2, 24), seed=17)
    w = torch.linspace(1.0, 2.0, 3, dtype=torch.float64)
    A = A0.clone().requires_grad_()
    trace = {}
    u, sv, vh = svd(LinearOperator.m(A), k=3, mode="uppest", method="gkl", min_eps=1e-13, ncv=20, trace=trace,
                    bck_options={"rtol": 1e-13, "atol": 1e-15})                 # (minres is the default here)
    assert trace["niter"] >= 1 and "handed_to" not in trace
    _loss(u, sv, vh, w).backward()
    Ar = A0.clone().requires_grad_()
    U, S, Vh = torch.linalg.svd(Ar, full_matrices=False)
    idx = torch.tensor([2, 1, 0])
    _loss(U[:, idx], S[idx], Vh[idx], w).backward()
    assert (A.grad - Ar.grad).abs().max() <= 1e-9 * Ar.grad.abs().max()
