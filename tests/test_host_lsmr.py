"""CPU: `linalg.lstsq` on operators in host memory (host_lsmr.py): the LSMR iteration in torch ops, its confirmation and
the implicit backward, against torch.linalg.pinv / the closed form in the same precision."""
import warnings
import pytest
import torch
from tests import test_gpu_lsmr as tg
from xitorch_amd import LinearOperator
from xitorch_amd._util import ConvergenceWarning
from xitorch_amd.linalg import lstsq, host_lsmr

DTYPES, IDS = tg.DTYPES, tg.IDS


def _tol(dtype):
    return 1e-12 if dtype in (torch.float64, torch.complex128) else 1e-5


def _solve(A, B, dtype, damp=0.0, **kw):
    trace = {}
    t = _tol(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        x = lstsq(LinearOperator.m(A.to(dtype)), B.to(dtype), damp=damp, atol=t, btol=t, max_niter=2000, trace=trace, **kw)
    return x.to(tg.hp_of(dtype)), trace


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(24, 10), (10, 24), (16, 16)], ids=["tall", "wide", "square"])
@pytest.mark.parametrize("damp", [0.0, 0.05])
@pytest.mark.parametrize("consistent", [False, True], ids=["inconsistent", "consistent"])
def test_against_pinv(dtype, shape, damp, consistent):
    A, B = tg.problem(dtype, shape, 30.0, consistent=consistent)
    x, trace = _solve(A, B, dtype, damp=damp)
    xs, fro, sv = tg.reference(A, B, damp)
    t = _tol(dtype)
    # forward error of a solution that meets S1 / S2 within the factor 2: 2 t |A|_F (|b| / sigma_min + |r| / sigma_min^2)
    nb = torch.linalg.vector_norm(B.expand(2, *B.shape[-2:]), dim=-2)
    smin = sv[:, -1:]
    lim = 2 * t * fro.unsqueeze(-1) * (nb / smin + nb / smin ** 2) + 2 * t * nb / smin
    err = torch.linalg.vector_norm(x - xs, dim=-2)
    assert bool((err <= lim).all()), (err, lim)
    assert all(c in (1, 2, 4, 5) for c in trace["stop_codes"])
    if consistent and damp == 0:
        assert all(c in (1, 5) for c in trace["stop_codes"]), trace


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_column_and_zero_block(dtype):
    A, B = tg.problem(dtype, (24, 10), 30.0)
    B = B.clone()
    B[:, 1] = 0
    x, trace = _solve(A, B, dtype)
    assert bool((x[:, :, 1] == 0).all())
    xs, _, _ = tg.reference(A, B, 0.0)
    assert float((x - xs).abs().max()) <= 1e3 * _tol(dtype) * float(xs.abs().max())
    z = lstsq(LinearOperator.m(A.to(dtype)), torch.zeros(24, 3, dtype=dtype))
    assert z.shape == (2, 10, 3) and bool((z == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rank_deficient_tall_gives_the_minimum_norm(dtype):
    A, B = tg.problem(dtype, (24, 10), 30.0, rank=6)
    x, trace = _solve(A, B, dtype)
    floor = float(torch.finfo(dtype).eps)
    assert tg.outside_range(A, x) <= 50 * floor
    xs = torch.linalg.pinv(A, rtol=1e-5) @ B
    assert float((x - xs).abs().max()) <= 1e4 * _tol(dtype) * float(xs.abs().max())


def test_broadcasting_of_batches():
    g = torch.Generator().manual_seed(1)
    A = torch.randn(3, 1, 12, 5, dtype=torch.float64, generator=g)
    B = torch.randn(2, 12, 4, dtype=torch.float64, generator=g)
    x = lstsq(LinearOperator.m(A), B, atol=1e-12, btol=1e-12)
    assert x.shape == (3, 2, 5, 4)
    xs = torch.linalg.pinv(A) @ B
    assert float((x - xs).abs().max()) <= 1e-9


def test_refusals():
    A = LinearOperator.m(torch.randn(12, 5, dtype=torch.float64))
    B = torch.randn(12, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="Unknown lstsq method"):
        lstsq(A, B, method="lsqr")
    with pytest.raises(RuntimeError, match="Mismatch shape"):
        lstsq(A, torch.randn(5, 2, dtype=torch.float64))
    for kw, word in ((dict(process_group=object()), "sharding"), (dict(E=torch.ones(2)), "shift"),
                     (dict(M=A), "metric"), (dict(precond=A), "preconditioner"), (dict(x0=B), "warm start")):
        with pytest.raises(NotImplementedError, match=word):
            lstsq(A, B, **kw)
    with pytest.raises(ValueError, match="damp"):
        lstsq(A, B, damp=-1.0)
    with pytest.raises(ValueError, match="damp"):
        lstsq(A, B, damp=torch.tensor(0.1))
    with pytest.raises(TypeError, match="unknown option"):
        lstsq(A, B, rtol=1e-3)
    assert lstsq(A, B, method="LSMR").shape == (5, 2)


def test_warnings():
    A, B = tg.problem(torch.float64, (24, 10), 1e4)
    op = LinearOperator.m(A)
    with pytest.warns(ConvergenceWarning, match="did not meet"):
        lstsq(op, B, atol=1e-14, btol=1e-14, max_niter=3)
    with pytest.warns(ConvergenceWarning, match="regularised"):
        lstsq(op, B, atol=1e-14, btol=1e-14, conlim=20.0)


def test_trace_and_call_counter():
    A, B = tg.problem(torch.float64, (24, 10), 30.0)
    before = host_lsmr.calls["lsmr"]
    _, trace = _solve(A, B, torch.float64)
    assert host_lsmr.calls["lsmr"] == before + 1
    for key in ("niter", "napply", "torch_applies", "host_reads", "restarts"):
        assert key in trace
    assert trace["napply"] >= 2 * trace["niter"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["f64", "c128"])
@pytest.mark.parametrize("shape,damp", [((12, 5), 0.0), ((5, 12), 0.0), ((12, 5), 0.2), ((5, 12), 0.2)],
                         ids=["column-rank", "row-rank", "tall-damped", "wide-damped"])
def test_gradcheck(dtype, shape, damp):
    g = torch.Generator().manual_seed(4)
    A = tg._randn(g, dtype, *shape).requires_grad_()
    B = tg._randn(g, dtype, shape[0], 2).requires_grad_()
    f = lambda A, B: lstsq(LinearOperator.m(A), B, damp=damp, atol=1e-13, btol=1e-13)
    assert torch.autograd.gradcheck(f, (A, B))


def test_bck_options_reach_the_backward_solves():
    g = torch.Generator().manual_seed(4)
    A = torch.randn(12, 5, dtype=torch.float64, generator=g, requires_grad=True)
    B = torch.randn(12, 2, dtype=torch.float64, generator=g, requires_grad=True)
    x = lstsq(LinearOperator.m(A), B, atol=1e-13, btol=1e-13, bck_options=dict(max_niter=1))
    with pytest.warns(ConvergenceWarning):
        x.sum().backward()
