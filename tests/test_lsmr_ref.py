"""CPU: the float64 restatement of LSMR (tests/lsmr_ref.py) is itself right, and its `check()` has teeth.

(a) the restated iteration agrees with torch.linalg.pinv in float64 on every solver case of tests/test_gpu_lsmr.py and
    stops there on S1 or S2 within that file's MAX_NITER (the evidence behind that constant);
(b) its estimates |rbar| and |Abar^H rbar| are the true ones, |Abar^H rbar| never grows, and the estimate of |A| stays
    below |A|_F;
(c) `check()` rejects every planted fault at every configuration tests/test_gpu_lsmr_kernels.py uses, and accepts the
    reference values rounded to the kernel dtype;
(d) the kernel restatements chained as the driver chains them reproduce the restated iteration;
(e) the iteration-level faults (no damping rotation, hbar updated after x, the u half run with length n) spoil the
    solution."""
import math
import pytest
import torch
from tests import lsmr_ref as lref
from tests import test_gpu_lsmr as tg


def _ops(A):
    """fwd / adj on (S, n) / (S, m) arrays for A (2, m, n) with S = 2 * ncols systems (member-major)"""
    nb = A.shape[0]

    def fwd(V):
        return torch.einsum("bij,bcj->bci", A, V.reshape(nb, -1, A.shape[2])).reshape(V.shape[0], A.shape[1])

    def adj(U):
        return torch.einsum("bij,bci->bcj", A.conj(), U.reshape(nb, -1, A.shape[1])).reshape(U.shape[0], A.shape[2])
    return fwd, adj


def _run(A, B, damp, tol, max_niter, fault=None, conlim=1e8):
    nb, m, n = A.shape
    rhs = B.expand(nb, m, B.shape[-1]).transpose(-2, -1).reshape(-1, m)
    fwd, adj = _ops(A)
    out = lref.iterate(fwd, adj, rhs, n, damp=damp, atol=tol, btol=tol, conlim=conlim, max_niter=max_niter, fault=fault)
    out["X"] = out["x"].reshape(nb, -1, n).transpose(-2, -1)
    return out


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", tg.CASES, ids=[c[0] for c in tg.CASES])
def test_solver_cases_converge_on_the_restated_iteration(case):
    _, dtype, shape, kappa, consistent, damp = case
    A, B = tg.problem(dtype, shape, kappa, consistent=consistent)
    t = tg.tol_of(dtype)
    out = _run(A, B, damp, t, tg.MAX_NITER)
    print("restated iteration: %d steps, codes %s" % (out["niter"], out["code"].tolist()))
    assert out["niter"] < tg.MAX_NITER
    assert all(c in (1.0, 2.0) for c in out["code"].tolist()), out["code"]
    tg.criteria(A, B, damp, out["X"], t, t, [int(c) for c in out["code"].tolist()],
                expect_s1=tg.expects_s1(shape, kappa, consistent, damp))


@pytest.mark.parametrize("kind", ["wide", "rank-deficient"])
def test_minimum_norm_of_the_restated_iteration(kind):
    dtype = torch.float64
    A, B = tg.problem(dtype, (40, 96), 1e2) if kind == "wide" else tg.problem(dtype, (96, 40), 1e2, rank=25)
    out = _run(A, B, 0.0, 1e-10, tg.MAX_NITER)
    assert all(c in (1.0, 2.0) for c in out["code"].tolist())
    assert tg.outside_range(A, out["X"]) <= 1e-12


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["real", "complex"])
@pytest.mark.parametrize("damp", [0.0, 0.05])
def test_estimates_are_the_true_norms(dtype, damp):
    A, B = tg.problem(dtype, (96, 40), 1e2)
    fro = torch.linalg.matrix_norm(A)
    prev = None
    for steps in (1, 2, 5, 11, 23):
        out = _run(A, B, damp, 0.0, steps, conlim=1e300)
        X = out["X"]
        r = B - A @ X
        g = A.conj().transpose(-2, -1) @ r - damp * damp * X
        nrbar = torch.sqrt(torch.linalg.vector_norm(r, dim=-2) ** 2 + (damp * torch.linalg.vector_norm(X, dim=-2)) ** 2)
        scale = float(torch.linalg.vector_norm(B, dim=-2).max())
        assert float((out["normr"].reshape(2, -1) - nrbar).abs().max()) <= 1e-9 * scale
        assert float((out["normar"].reshape(2, -1) - torch.linalg.vector_norm(g, dim=-2)).abs().max()) <= 1e-9 * scale
        # (the capped estimate: the plain Frobenius norm of the bidiagonal is 2.54 against |A|_F = 2.18 at 23 steps)
        assert bool((out["normA"].reshape(2, -1) <= fro.unsqueeze(-1) * (1 + 1e-12)).all())
        if prev is not None:
            assert bool((out["normar"] <= prev * (1 + 1e-9)).all()), "|A^H r| must not grow"
        prev = out["normar"]


# ------------------------------------------------------------------------------------------------ (c)
def _got(ref):
    return {n: v[0] for n, v in ref.items() if isinstance(v, tuple)}


def _good(ref):
    return {n: v for n, v in ref.items() if isinstance(v, tuple)}


@pytest.mark.parametrize("dtype,cfg", lref.CASES, ids=lref.CASE_IDS)
def test_check_rejects_every_fault(dtype, cfg):
    N, S, extra, nblk = cfg
    c = lref.Case(dtype, N, S, extra, nblk, seed=N + S, other="rand")
    env = c.env
    kernels = {"init": c.ref_init, "bidiag": lambda fault=None: c.ref_bidiag(0, fault),
               "bidiag_v": lambda fault=None: c.ref_bidiag(1, fault), "update": c.ref_update}
    seen = set()
    for name, fn in kernels.items():
        good = _good(fn())
        rounded = {n: v.to(env.rdtype).to(torch.float64) for n, (v, _) in good.items() if n not in ("state", "run")}
        lref.check(rounded, {n: good[n] for n in rounded}, dtype, what=name)
        for fault in lref.FAULTS:
            kname = "bidiag" if name == "bidiag_v" else name
            if not lref.applicable(env, fault, kname) or (fault == "u_len_n" and name != "bidiag"):
                continue
            if fault == "no_damp" and not c.ref_update()["reg"].any():
                continue
            seen.add(fault)
            bad = _got(fn(fault))
            with pytest.raises(AssertionError):
                lref.check(bad, good, dtype, what="%s fault=%s" % (name, fault))
    want = set(lref.FAULTS)
    if env.n % env.rctx.vn == 0:
        want.discard("drop_tail")
    if N < 4:
        want.discard("u_len_n")
    assert seen == want


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["real", "complex"])
@pytest.mark.parametrize("damp", [0.0, 0.3])
def test_chained_kernel_restatements_are_the_iteration(dtype, damp):
    g = torch.Generator().manual_seed(3)
    m, n, S, steps = 29, 17, 2, 9
    A = lref.spectrum_matrix(g, dtype, m, n, 30.0)[0]
    B = tg._randn(g, dtype, S, m)
    fwd, adj = (lambda V: V @ A.T), (lambda U: U @ A.conj())
    tol = dict(damp=damp, atol=0.0, btol=0.0, conlim=1e300)
    want = lref.iterate(fwd, adj, B, n, max_niter=steps, **tol)
    nbu, nbv = 3, 2
    eu, ev = lref.Env(dtype, S, m, nbu), lref.Env(dtype, S, n, nbv)

    def parts(val, nblk):
        P = torch.full((S, 64), math.nan, dtype=torch.float64)
        P[:, :nblk] = 0
        P[:, 0] = val
        return P

    state = torch.full((2, S, lref.NST), math.nan, dtype=torch.float64)
    sq = lambda t: (t * t).sum(-1)
    uh = eu.vec(B)
    o = lref.init(eu, uh, parts(sq(uh), nbu), 0)
    state[0] = o["state"][0]
    Pu = parts(sq(uh), nbu)
    vh, h, hbar, x = (torch.zeros(S, ev.n, dtype=torch.float64) for _ in range(4))
    Px = parts(torch.zeros(S, dtype=torch.float64), nbv)
    k = 0

    def v_half_and_update(k, vh, h, hbar, x, Px):
        Op = ev.vec(adj(eu.unvec(uh)))
        bd = lref.bidiag(ev, Op, vh, Pu, nbu, state, 1, k)
        vh = bd["y"][0]
        Pv = parts(bd["Pout"][0], nbv)
        up = lref.update(ev, vh, h, hbar, x, Pu, nbu, Pv, Px, state, k, **tol)
        state[(k + 1) & 1] = up["state"][0]
        return vh, up["h"][0], up["hbar"][0], up["x"][0], parts(up["Pxout"][0], nbv), Pv

    vh, h, hbar, x, _, Pv = v_half_and_update(k, vh, h, hbar, x, Px)
    k += 1
    for _ in range(steps):
        Op = eu.vec(fwd(ev.unvec(vh)))
        bd = lref.bidiag(eu, Op, uh, Pv, nbv, state, 0, k)
        uh = bd["y"][0]
        Pu = parts(bd["Pout"][0], nbu)
        vh, h, hbar, x, Px, Pv = v_half_and_update(k, vh, h, hbar, x, Px)
        k += 1
    got = ev.unvec(x)
    # (two float64 evaluation orders, nine steps at kappa = 30: rounding differences of 1e-16 kappa^2 per step)
    assert float((got - want["x"]).abs().max()) <= 1e-10 * float(want["x"].abs().max())
    st = state[k & 1]
    assert float((st[:, lref.NORMR] - want["normr"]).abs().max()) <= 1e-10 * float(B.norm())
    assert float((st[:, lref.NORMAR] - want["normar"]).abs().max()) <= 1e-10 * float(B.norm())


# ------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("fault", ["no_damp", "hbar_after_x", "u_len_n"])
def test_iteration_faults_spoil_the_solution(fault):
    A, B = tg.problem(torch.float64, (96, 40), 1e2)
    damp = 0.05
    xs, _, _ = tg.reference(A, B, damp)
    good = _run(A, B, damp, 1e-10, tg.MAX_NITER)
    bad = _run(A, B, damp, 1e-10, tg.MAX_NITER, fault=fault)
    assert float((good["X"] - xs).abs().max()) <= 1e-7 * float(xs.abs().max())
    assert float((bad["X"] - xs).abs().max()) >= 1e-4 * float(xs.abs().max())
