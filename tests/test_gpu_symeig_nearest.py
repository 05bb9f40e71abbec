"""-m gpu: symeig(mode="nearest", sigma=, method="chebfsi") on the HIP kernels — the solver cases of
tests/test_host_symeig_nearest.py on the device (same matrices, same conditions and bounds: tests/nearest_cases.py) for
dense, CSR, banded and user `_mv` operators in four dtypes, agreement with the host twin, and what the device path
reports and must not touch.  (On the parent commit the mode is unknown and sigma is not an option.)"""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linalg import symeig, host_eig
from tests import nearest_cases as nc

pytestmark = pytest.mark.gpu
F64, F32, C128, C64 = nc.DTYPES
NATIVE_DENSE = ("K1s", "K1sw", "K1w", "K1wr", "K1")


@pytest.fixture(autouse=True)
def _no_convergence_warnings():
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        yield


_host = {}


def _host_twin(name, dtype):
    """the host twin's eigenvalues of a case, computed once"""
    key = (name, dtype)
    if key not in _host:
        build, kind, sigma, neig, _ = nc.CASES[name]
        ev, _X = nc.solve(nc.make_operator(kind, build(dtype), torch.device("cpu")), neig, sigma, dtype)
        _host[key] = ev
    return _host[key]


SOLVER_CASES = [(n, d) for n in ("dense257", "dense200", "lap16x17_csr", "lap16x16_7", "tridiag300", "tridiag300_mv")
                for d in nc.DTYPES] + [("lap16x16_5", F64), ("lap16x16_5", C64), ("dense257_below", F64),
                                       ("dense257_below", C64), ("dense257_above", F32), ("dense257_above", C128)]
CASE_IDS = ["%s-%s" % (n, nc.IDS[nc.DTYPES.index(d)]) for n, d in SOLVER_CASES]
# what PanelOperator reports: real dense operators name their K1 form; complex dense ones run on the Hermitian K1
# route, which records no name (None: in any case not the generic torch apply); there is no complex banded kernel
KERNEL_OF = {("sparse", False): ("csr",), ("sparse", True): ("csr",), ("banded", False): ("banded",),
             ("banded", True): ("generic",), ("mv", False): ("generic",), ("mv", True): ("generic",),
             ("dense", False): NATIVE_DENSE, ("dense", True): (None,)}


@pytest.mark.parametrize("name,dtype", SOLVER_CASES, ids=CASE_IDS)
def test_chebfsi_nearest_on_the_device(dev, name, dtype):
    build, kind, sigma, neig, projector = nc.CASES[name]
    A = build(dtype)
    before = dict(host_eig.calls)
    tr = {}
    ev, X = nc.solve(nc.make_operator(kind, A, dev), neig, sigma, dtype, trace=tr)
    assert dict(host_eig.calls) == before, "a device run reached the host twin"
    assert ev.is_cuda and X.is_cuda
    print("%s: %d iterations, %d applies, degrees %s, %s" % (name, tr["niter"], tr["napply"], tr["degrees"],
                                                            tr["panel_kernel"]))
    nc.check(A, sigma, neig, ev, X, dtype, projector=projector, what=name)
    assert tr["panel_kernel"] in KERNEL_OF[(kind, dtype.is_complex)], tr["panel_kernel"]
    assert len(tr["degrees"]) == tr["niter"] <= nc.MAX_NITER and tr["degrees"][0] == 20 and not tr["degree_capped"]
    assert tr["napply"] >= sum(tr["degrees"]) + tr["niter"]
    # against the host twin: both within the eigenvalue bound of the float64 selection, so within it of each other
    ev_h = _host_twin(name, dtype)
    n = A.shape[-1]
    lam_max = float(torch.linalg.eigvalsh(A.to(torch.complex128 if dtype.is_complex else torch.float64)).abs().max())
    bound = (n ** 0.5) * nc.min_eps(dtype) + n * torch.finfo(nc.REAL_OF[dtype]).eps * lam_max
    assert float((ev.cpu().double() - ev_h.double()).abs().max()) <= bound


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_sigma_outside_the_spectrum_gives_the_end_of_it(dev, dtype):
    A = nc.dense_matrix(dtype, 257)
    op = xa.LinearOperator.m(A.to(dev), True)
    bound = (257 ** 0.5) * nc.min_eps(dtype) + 257 * torch.finfo(dtype).eps * 2.0
    for sigma, mode in ((-5.0, "lowest"), (7.0, "uppest")):
        ev, _ = nc.solve(op, 4, sigma, dtype)
        ev_end, _ = symeig(op, 4, mode, method="exacteig")
        assert float((ev - ev_end).abs().max()) <= bound


def test_batch_of_three_with_a_sigma_tensor(dev):
    mats = [nc.dense_matrix(F64, 257, seed=s) for s in (0, 1, 2)]
    sigmas = torch.tensor([0.62, -0.3, 1.41], dtype=torch.float64)
    tr = {}
    ev, X = nc.solve(xa.LinearOperator.m(torch.stack(mats).to(dev), True), 4, sigmas.to(dev), F64, trace=tr)
    assert ev.shape == (3, 4) and X.shape == (3, 257, 4)
    for b in range(3):
        nc.check(mats[b], float(sigmas[b]), 4, ev[b], X[b], F64, what="member %d" % b)
    assert tr["sigma_centre"] == pytest.approx(sigmas.tolist()) and tr["panel_kernel"] in NATIVE_DENSE
    # sigma may live on the host as well
    ev2, _ = nc.solve(xa.LinearOperator.m(torch.stack(mats).to(dev), True), 4, sigmas, F64)
    assert torch.equal(ev, ev2)


def test_fixed_degree_and_cap_on_the_device(dev):
    A = nc.dense_matrix(F64, 257)
    op = xa.LinearOperator.m(A.to(dev), True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", xa.ConvergenceWarning)
        tr = {}
        symeig(op, 4, "nearest", method="chebfsi", sigma=0.62, filter_degree=37, max_niter=3, min_eps=1e-30, trace=tr)
        assert tr["degrees"] == [37, 37, 37] and tr["napply"] == 12 + 3 * 38
        tr = {}
        symeig(op, 4, "nearest", method="chebfsi", sigma=0.62, filter_degree=1, max_niter=2, min_eps=1e-30, trace=tr)
        assert tr["degrees"] == [1, 1]
        tr = {}
        symeig(op, 4, "nearest", method="chebfsi", sigma=0.62, max_degree=50, max_niter=4, min_eps=1e-30, trace=tr)
        assert tr["degrees"][0] == 20 and tr["degrees"][-1] == 50 and tr["degree_capped"]


def test_refusals_and_handover_on_the_device(dev):
    A = nc.dense_matrix(F64, 200)
    op = xa.LinearOperator.m(A.to(dev), True)
    with pytest.raises(ValueError, match="sigma"):
        symeig(op, 3, "nearest", method="chebfsi")
    for method in ("davidson", "lobpcg"):
        with pytest.raises(NotImplementedError, match="chebfsi"):
            symeig(op, 3, "nearest", method=method, sigma=0.5)
    with pytest.raises(NotImplementedError, match="davidson"):
        symeig(op, 3, "nearest", method="chebfsi", sigma=0.5,
               M=xa.LinearOperator.m(torch.eye(200, dtype=torch.float64, device=dev), True))
    small = nc.dense_matrix(F64, 20)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(small.to(dev), True), 3, "nearest", method="chebfsi", sigma=0.55, trace=tr)
    assert tr["handed_to"] == "exacteig"
    nc.check(small, 0.55, 3, ev, X, F64, what="handed over")
    ev_x, X_x = symeig(op, 4, "nearest", method="exacteig", sigma=0.62)
    nc.check(A, 0.62, 4, ev_x, X_x, F64, what="exacteig on the device")


def test_backward_matches_exacteig_on_the_device(dev):
    """order 40, 3 pairs, float64 (a block of 11: no hand-off), 1e-6 relative as the other symeig gradient tests"""
    A0 = nc.dense_matrix(F64, 40)
    nc.reference(A0, 0.62, 3)
    g = torch.Generator().manual_seed(11)
    D = torch.randn(40, 40, dtype=torch.float64, generator=g)
    D = ((D + D.T) * 0.5).to(dev)
    grads = {}
    for method, kw in (("chebfsi", dict(min_eps=1e-11, max_niter=60)), ("exacteig", {})):
        a = A0.to(dev).requires_grad_()
        As = (a + a.T) * 0.5
        tr = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", xa.ConvergenceWarning)
            ev, X = symeig(xa.LinearOperator.m(As, True), 3, "nearest", method=method, sigma=0.62,
                           **(dict(kw, trace=tr) if kw else {}))
        if kw:
            assert "handed_to" not in tr and tr["w"] == 11
        loss = (ev * torch.arange(1, 4, dtype=torch.float64, device=dev)).sum() + torch.einsum("ni,nm,mi->", X, D, X)
        grads[method], = torch.autograd.grad(loss, a)
    ga, gb = grads["chebfsi"], grads["exacteig"]
    assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max())
