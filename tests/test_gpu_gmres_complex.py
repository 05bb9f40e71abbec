"""-m gpu: solve(method="gmres") on COMPLEX device operators (native_krylov.gmres on xk_gmres_c.hip): the host cases of
tests/test_host_gmres_complex.py on the device under the same residual rule, `arnoldi_steps` equal to the host driver's
and to the textbook's on the factor-2 cases, a complex-shifted 7-point stencil in CSR, the implicit backward against
finite differences, resid_calc_every=, the lazy limit of the un-restarted basis, two gloo ranks on one GPU, and the
guarantee that a device operator reaches neither the host driver nor a torch-expression Gram / lstsq."""
import os
import socket
import time
import warnings
import pytest
import torch
import torch.multiprocessing as mp
import xitorch_amd as xa
from xitorch_amd.linalg import solve, host_krylov, native_krylov as nk
from xitorch_amd._capi import NativeLibraryError
from tests import gmres_complex_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _solve(case, data, device=DEV, method="gmres", **kw):
    Aop, B, E, Mop = C.operators(case, data, device)
    tr = {}
    X = solve(Aop, B, E, Mop, method=method, posdef=True, trace=tr, **kw)
    return X, tr


@pytest.mark.parametrize("case", C.RULE_CASES, ids=[c["name"] for c in C.RULE_CASES])
def test_rule(case):
    data = C.make(case)
    rt, at = C.RTOL[case["dtype"]], C.ATOL[case["dtype"]]
    before = dict(host_krylov.calls)
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X, tr = _solve(case, data, rtol=rt, atol=at)
    assert dict(host_krylov.calls) == before
    assert X.is_cuda and X.dtype == case["dtype"] and tr["converged"]
    r, lim = C.residual_rule(case, data, X, rt, at)
    print("%s: max |r| / limit %.3f, steps %d" % (case["name"], float((r / lim).max()), tr["arnoldi_steps"]))
    assert bool((r <= lim).all())


@pytest.mark.parametrize("case", C.STEP_CASES, ids=[c["name"] for c in C.STEP_CASES])
def test_arnoldi_steps_equal_host_and_textbook(case):
    data = C.make(case)
    steps, ok = C.textbook_steps(case, data, case["rtol"], C.STEP_ATOL)
    assert ok
    Xd, trd = _solve(case, data, rtol=case["rtol"], atol=C.STEP_ATOL)
    Xh, trh = _solve(case, data, device="cpu", rtol=case["rtol"], atol=C.STEP_ATOL)
    assert trd["converged"] and trd["arnoldi_steps"] == trh["arnoldi_steps"] == steps
    r, lim = C.residual_rule(case, data, Xd, case["rtol"], C.STEP_ATOL)
    assert bool((r <= lim).all())


@pytest.mark.parametrize("name", ["dense_c128", "csr_c64", "dense_EM_c128"])
def test_restart(name):
    case = next(c for c in C.RULE_CASES if c["name"] == name)
    data = C.make(case)
    rt, at = C.RTOL[case["dtype"]], C.ATOL[case["dtype"]]
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X, tr = _solve(case, data, rtol=rt, atol=at, restart=7, max_niter=400)
    assert tr["converged"] and tr["restarts"] >= 1
    r, lim = C.residual_rule(case, data, X, rt, at)
    assert bool((r <= lim).all())


@pytest.mark.parametrize("name", ["dense_c128", "mv_c64", "csr_E_c128"])
def test_resid_calc_every(name):
    case = next(c for c in C.RULE_CASES if c["name"] == name)
    data = C.make(case)
    rt, at = C.RTOL[case["dtype"]], C.ATOL[case["dtype"]]
    X1, tr1 = _solve(case, data, rtol=rt, atol=at)
    X5, tr5 = _solve(case, data, rtol=rt, atol=at, resid_calc_every=5)
    assert tr5["converged"] and tr5["napply"] < tr1["napply"]
    r, lim = C.residual_rule(case, data, X5, rt, at)
    assert bool((r <= lim).all())
    # the same accepted iterate within the rule: both satisfy it, so they differ by at most two thresholds' worth
    # (x5 - x1 = (A - e_c I)^-1 (r1 - r5) per column c, |r1|, |r5| <= lim)
    d = torch.linalg.vector_norm((X5 - X1).cpu().to(torch.complex128), dim=-2)
    eye = torch.eye(case["n"], dtype=torch.complex128)
    for c in range(data["B"].shape[-1]):
        Ac = data["A"] if data["E"] is None else data["A"] - data["E"][c] * eye
        Ainv = torch.linalg.matrix_norm(torch.linalg.inv(Ac), ord=2)
        assert bool(d[c] <= 2 * lim[c] * Ainv), (c, float(d[c]), float(lim[c]), float(Ainv))


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_zero_rhs(dtype):
    case = dict(kind="dense", dtype=dtype, n=20, seed=50, ncols=2)
    data = C.make(case)
    data["B"] = torch.zeros_like(data["B"])
    X, tr = _solve(case, data)
    assert X.is_cuda and X.dtype == dtype and tuple(X.shape) == (20, 2) and bool((X == 0).all()) and tr == {}


def test_not_converged_returns_the_best_iterate_with_a_warning():
    case = dict(kind="dense", dtype=torch.complex128, n=48, seed=1)
    data = C.make(case)
    with pytest.warns(xa.ConvergenceWarning):
        X, tr = _solve(case, data, rtol=1e-12, atol=1e-30, max_niter=6)
    assert not tr["converged"] and tr["arnoldi_steps"] == 5
    r, _ = C.residual_rule(case, data, X, 0.0, 0.0)
    bn = torch.linalg.vector_norm(data["B"], dim=-2)
    assert abs(float(r.max()) - tr["best_resid"]) <= 1e-12 * float(bn.max()) and bool((r < bn).all())


def _helmholtz(n, k2, eta, dtype):
    """7-point stencil of -Laplace on an n^3 grid (Dirichlet) in CSR, and the shift E = k^2 + i eta (A - E I)"""
    idx = torch.arange(n ** 3).reshape(n, n, n)
    rows, cols, vals = [idx.reshape(-1)], [idx.reshape(-1)], [torch.full((n ** 3,), 6.0)]
    for d in range(3):
        a = idx.narrow(d, 0, n - 1).reshape(-1)
        b = idx.narrow(d, 1, n - 1).reshape(-1)
        rows += [a, b]
        cols += [b, a]
        vals += [torch.full((a.numel(),), -1.0)] * 2
    t = torch.sparse_coo_tensor(torch.stack([torch.cat(rows), torch.cat(cols)]), torch.cat(vals).to(dtype),
                                (n ** 3, n ** 3)).coalesce().to_sparse_csr()
    return t, torch.tensor([complex(k2, eta)], dtype=dtype)


def test_helmholtz_csr_complex_shift():
    """(-Laplace - (k^2 + i eta)) x = b: complex symmetric, not Hermitian — minres refuses, gmres(40) converges; the
    applies of gmres(40) and of complex bicgstab on the same system are printed, no ratio is asserted"""
    dtype, n = torch.complex128, 24
    t, E = _helmholtz(n, 0.9, 0.3, dtype)
    Aop = xa.SparseLinearOperator(t.crow_indices().to(DEV), t.col_indices().to(DEV), t.values().to(DEV),
                                  tuple(t.shape), is_hermitian=True)
    g = torch.Generator().manual_seed(70)
    B = C._crand(g, n ** 3, 1).to(DEV)
    Ed = E.to(DEV)
    with pytest.raises(RuntimeError):
        solve(Aop, B, Ed, method="minres")
    out = {}
    for meth, kw in (("gmres", dict(restart=40, max_niter=4000)), ("bicgstab", dict(max_niter=4000))):
        tr = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", xa.ConvergenceWarning)
            X = solve(Aop, B, Ed, method=meth, posdef=True, rtol=1e-8, atol=1e-30, trace=tr, **kw)
        torch.cuda.synchronize()
        out[meth] = (tr, time.perf_counter() - t0, X)
        print("helmholtz n=%d^3 %s: converged %s niter %d napply %d best %.3e  %.3f s"
              % (n, meth, tr["converged"], tr["niter"], tr["napply"], tr["best_resid"], time.perf_counter() - t0))
    tr, _, X = out["gmres"]
    assert tr["converged"]
    Xh = X.cpu()
    xg = torch.nn.functional.pad(Xh.reshape(n, n, n), (1, 1, 1, 1, 1, 1))      # the stencil again, on the padded grid
    Ax = 6.0 * xg[1:-1, 1:-1, 1:-1] - xg[:-2, 1:-1, 1:-1] - xg[2:, 1:-1, 1:-1] - xg[1:-1, :-2, 1:-1] \
        - xg[1:-1, 2:, 1:-1] - xg[1:-1, 1:-1, :-2] - xg[1:-1, 1:-1, 2:]
    r = B.cpu() - (Ax.reshape(-1, 1) - Xh * E)
    bn = float(torch.linalg.vector_norm(B))
    # gamma = 2 * 7 + 5 for a 7-term row with a shift (gmres_complex_cases.residual_rule)
    slack = 19 * C.U128 * ((12.0 + abs(E.item())) * float(Xh.abs().sum()) + bn)
    assert float(torch.linalg.vector_norm(r)) <= 1e-8 * bn + slack


def test_backward_against_finite_differences():
    g = torch.Generator().manual_seed(61)
    n = 12
    A0 = (0.3 * C._crand(g, n, n) + torch.eye(n, dtype=torch.complex128) * (2.0 + 0.5j)).to(DEV).requires_grad_()
    B0 = C._crand(g, n, 2).to(DEV).requires_grad_()
    W = C._crand(g, n, 2).to(DEV)
    opts = dict(method="gmres", posdef=True, rtol=1e-13, atol=1e-30, restart=n, max_niter=100)

    def loss(A, B):
        X = solve(xa.LinearOperator.m(A, is_hermitian=False), B, bck_options=dict(opts), **opts)
        return (X * W.conj()).real.sum()
    before = dict(host_krylov.calls)
    gA, gB = torch.autograd.grad(loss(A0, B0), (A0, B0))
    assert dict(host_krylov.calls) == before
    # central differences along random complex directions: dL = Re <grad, d> for torch's convention (grad = dL/d conj)
    for P, gP, which in ((A0, gA, 0), (B0, gB, 1)):
        d = C._crand(g, *P.shape).to(DEV)
        h = 1e-6
        args = lambda s: (A0.detach() + s * d, B0.detach()) if which == 0 else (A0.detach(), B0.detach() + s * d)
        fd = (loss(*args(h)) - loss(*args(-h))).item() / (2 * h)
        an = (gP.conj() * d).real.sum().item()
        # truncation h^2 |L'''| ~ 1e-12 and cancellation u |L| / h ~ 1e-10 * |L|
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (which, fd, an)


def test_lazy_limit_message_through_the_argument_check():
    n = 4200
    A = xa.LinearOperator.m(torch.eye(n, dtype=torch.complex64, device=DEV) * (1 + 1j), is_hermitian=False)
    B = torch.ones(n, 1, dtype=torch.complex64, device=DEV)
    with pytest.raises(NativeLibraryError, match="4096"):
        nk.gmres(A, B, restart=4097, max_niter=5000)
    # the un-restarted default only fails if a run gets that far: this one converges in one step
    tr = {}
    X = nk.gmres(A, B, trace=tr)
    assert tr["converged"] and tr["arnoldi_steps"] == 1
    # real operators keep their limit
    Ar = xa.LinearOperator.m(torch.eye(16, dtype=torch.float32, device=DEV), is_hermitian=False)
    with pytest.raises(NativeLibraryError, match="8192"):
        nk.gmres(Ar, torch.ones(16, 1, dtype=torch.float32, device=DEV), restart=8193, max_niter=9000)


def test_device_path_reaches_no_host_driver_lstsq_or_torch_gram(monkeypatch):
    case = next(c for c in C.RULE_CASES if c["name"] == "dense_EM_c128")
    data = C.make(case)
    before = dict(host_krylov.calls)

    def forbidden(name):
        def f(*a, **k):
            raise AssertionError("%s reached from the device path" % name)
        return f
    monkeypatch.setattr(torch.linalg, "lstsq", forbidden("torch.linalg.lstsq"))
    monkeypatch.setattr(host_krylov, "gmres", forbidden("host_krylov.gmres"))
    monkeypatch.setattr(host_krylov, "_coldot", forbidden("host_krylov._coldot"))
    for n in ("einsum", "bmm", "baddbmm", "vdot", "dot"):
        monkeypatch.setattr(torch, n, forbidden("torch." + n))
    X, tr = _solve(case, data, rtol=1e-9, atol=1e-14)
    csr = next(c for c in C.RULE_CASES if c["name"] == "csr_c64")
    _solve(csr, C.make(csr), rtol=1e-4, atol=1e-8, restart=5, max_niter=200)
    assert tr["converged"] and dict(host_krylov.calls) == before
    # a host driver refuses a device operator; without the library a device call fails
    monkeypatch.undo()
    Aop, B, E, Mop = C.operators(case, data, DEV)
    with pytest.raises(NativeLibraryError):
        host_krylov.gmres(Aop, B, E, Mop)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, results):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from xitorch_amd import dist as xd
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(80)
        Bt, n = 4, 64
        A = (0.5 * C._crand(g, Bt, n, n) / n ** 0.5 + torch.eye(n, dtype=torch.complex128) * (1.0 + 0.3j))
        # members converge at different speeds: the slowest decides for everybody
        A = A * torch.linspace(1.0, 1.5, Bt, dtype=torch.float64).reshape(Bt, 1, 1)
        Bm = C._crand(g, Bt, n, 2)
        lo, hi = xd.shard_range(Bt, world, rank)
        tr_f, tr_s = {}, {}
        Xf = solve(xa.LinearOperator.m(A.to(dev), False), Bm.to(dev), method="gmres", posdef=True, rtol=1e-9,
                   trace=tr_f)
        Xs = solve(xa.LinearOperator.m(A[lo:hi].contiguous().to(dev), False), Bm[lo:hi].to(dev), method="gmres",
                   posdef=True, rtol=1e-9, trace=tr_s, process_group=dist.group.WORLD)
        results[rank] = dict(steps=(tr_s["arnoldi_steps"], tr_f["arnoldi_steps"]), conv=tr_s["converged"],
                             err=(Xs - Xf[lo:hi]).abs().max().item())
    finally:
        dist.destroy_process_group()


def test_sharded_two_ranks_one_gpu():
    world = 2
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    results = mgr.dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, results)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:                            # never leave a worker behind with the GPU open
        p.kill()
        p.join(30)
    assert not hung and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    for rank in range(world):
        r = results[rank]
        assert r["conv"] and r["steps"][0] == r["steps"][1], r
        assert r["err"] < 1e-9, r
