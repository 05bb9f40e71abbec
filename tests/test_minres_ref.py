"""CPU: the float64 restatement of MINRES (tests/minres_ref.py) is itself right, and its `check()` has teeth.

(a) the restated iteration solves Hermitian definite, indefinite and complex systems (against torch.linalg.solve);
(b) after k steps its residual is the least-squares minimum over the explicit Krylov basis -- the defining property
    of MINRES, and what un-restarted GMRES computes on such operators;
(c) `check()` rejects every planted fault at every configuration tests/test_gpu_minres_kernels.py uses;
(d) the kernel restatements chained as the driver chains them reproduce the restated iteration;
(e) the inputs of tests/test_gpu_minres.py are such that the restated iteration alone meets that
    file's criterion, and the drift of the singular-system answer out of the null vector's complement is measured."""
import math
import pytest
import torch
from tests import krylov_ref as kref
from tests import minres_ref as mref


def _spectrum(kind, n):
    if kind == "definite":
        return torch.linspace(1.0, 50.0, n, dtype=torch.float64)
    ev = torch.linspace(0.1, 30.0, n, dtype=torch.float64) - 3.05          # ~10 % negative eigenvalues
    return ev


def _rhs(g, dtype, S, n):
    if dtype.is_complex:
        return torch.complex(torch.randn(S, n, dtype=torch.float64, generator=g),
                             torch.randn(S, n, dtype=torch.float64, generator=g))
    return torch.randn(S, n, dtype=torch.float64, generator=g)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["real", "complex"])
@pytest.mark.parametrize("kind", ["definite", "indefinite"])
@pytest.mark.parametrize("precond", [False, True], ids=["plain", "precond"])
def test_iteration_solves(dtype, kind, precond):
    g = torch.Generator().manual_seed(11)
    n, S, rtol = 80, 3, 1e-10
    ev = _spectrum(kind, n)
    A, _ = mref.hermitian(g, dtype, n, ev)
    B = _rhs(g, dtype, S, n)
    pre = None
    if precond:
        d = 1.0 / (1.0 + torch.rand(n, dtype=torch.float64, generator=g))   # a positive diagonal preconditioner
        pre = lambda R: R * d
    stop = rtol * B.norm(dim=-1)
    out = mref.iterate(lambda V: V @ A.T, B, stop, 4 * n, pre=pre)
    Xref = torch.linalg.solve(A, B.T).T
    kappa = float(ev.abs().max() / ev.abs().min())
    err = (out["x"] - Xref).norm(dim=-1)
    if precond:
        # the recurrence then measures the P-norm of the residual; P's spectrum lies in [1/2, 1]
        kappa *= 2
    assert bool((err <= 2 * rtol * kappa * Xref.norm(dim=-1)).all()), (err, out["niter"])
    assert out["niter"] < 4 * n
    h = out["hist"]
    assert all(h[i + 1] <= h[i] * (1 + 1e-12) for i in range(len(h) - 1)), "phibar must not grow"


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["real", "complex"])
@pytest.mark.parametrize("n", [13, 24])
def test_residual_is_the_krylov_least_squares_minimum(dtype, n):
    g = torch.Generator().manual_seed(5 + n)
    ev = torch.linspace(-2.0, 5.0, n, dtype=torch.float64) + 0.13
    A, _ = mref.hermitian(g, dtype, n, ev)
    B = _rhs(g, dtype, 2, n)
    for k in range(1, 13):
        out = mref.iterate(lambda V: V @ A.T, B, None, None, steps=k)
        for s in range(2):
            b = B[s]
            cols, q = [], b
            for _ in range(k):                              # A K_k(A, b) = span{A b, ..., A^k b}
                q = A @ q
                cols.append(q)
            AK, _ = torch.linalg.qr(torch.stack(cols, -1))   # orthonormal basis: the projection is well conditioned
            rmin = (b - AK @ (AK.conj().T @ b)).norm()
            rk = (b - A @ out["x"][s]).norm()
            tol = 1e-9 * b.norm()
            assert abs(float(rk - rmin)) <= float(tol), (k, s, float(rk), float(rmin))
            assert abs(float(out["phibar"][s] - rk)) <= float(tol), "phibar is the residual norm"


# ------------------------------------------------------------------------------------------------ (c)
def _faulty_got(ref):
    return {n: v[0] for n, v in ref.items() if isinstance(v, tuple)}


def _good(ref):
    return {n: v for n, v in ref.items() if isinstance(v, tuple)}


@pytest.mark.parametrize("dtype,cfg", mref.CASES, ids=mref.CASE_IDS)
def test_check_rejects_every_fault(dtype, cfg):
    N, S, extra, nblk = cfg
    c = mref.Case(dtype, N, S, extra, nblk, seed=N + S)
    env = c.env
    kernels = {"alpha_dot": c.ref_alpha_dot, "init": c.ref_init, "lanczos": c.ref_lanczos, "update": c.ref_update}
    seen = set()
    for name, fn in kernels.items():
        good = _good(fn())
        # the reference values rounded to the kernel dtype pass: the bounds leave room for a correct kernel
        rounded = {n: v.to(env.rdtype).to(torch.float64) for n, (v, _) in good.items() if n != "state"}
        mref.check(rounded, {n: good[n] for n in rounded}, dtype, what=name)
        for fault in mref.FAULTS:
            if not mref.applicable(env, fault, name):
                continue
            seen.add(fault)
            bad = _faulty_got(fn(fault))
            with pytest.raises(AssertionError):
                mref.check(bad, good, dtype, what="%s fault=%s" % (name, fault))
    want = set(mref.FAULTS)
    if not env.cplx:
        want.discard("noconj")
    if env.n % env.rctx.vn == 0:
        want.discard("drop_tail")
    assert seen == want


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["real", "complex"])
def test_chained_kernel_restatements_are_the_iteration(dtype):
    g = torch.Generator().manual_seed(3)
    n, S, nblk, steps = 37, 2, 3, 9
    A, _ = mref.hermitian(g, dtype, n, torch.linspace(-1.0, 4.0, n, dtype=torch.float64) + 0.21)
    B = _rhs(g, dtype, S, n)
    env = mref.Env(dtype, S, n, nblk)
    want = mref.iterate(lambda V: V @ A.T, B, None, None, steps=steps)

    def parts(val):
        """a partial array holding `val` (S,) real in slot 0, zeros in the other used slots"""
        P = torch.full((S, 64, 2) if env.cplx else (S, 64), math.nan, dtype=torch.float64)
        P[:, :nblk] = 0
        if env.cplx:
            P[:, 0, 0] = val
        else:
            P[:, 0] = val
        return P

    dot = lambda a, b: (a.conj() * b).sum(-1).real
    state = torch.full((2, S, mref.NST), math.nan, dtype=torch.float64)
    o = mref.init(env, env.vec(B), parts(dot(B, B)), 0)
    state[0] = o["state"][0]
    v, r2 = o["v"][0], env.vec(B)
    r1, w1, w2, x = (torch.zeros_like(v) for _ in range(4))
    for k in range(steps):
        Av = env.vec(env.unvec(v) @ A.T)
        Pa = parts(dot(env.unvec(v), env.unvec(Av)))
        lz = mref.lanczos(env, Av, r2, r1, Pa, state, k)
        r1, r2 = r2, lz["r1"][0]
        Pb = torch.full((S, 64), math.nan, dtype=torch.float64)
        Pb[:, :nblk] = 0
        Pb[:, 0] = lz["Pbeta"][0]
        up = mref.update(env, v, r2, w1, w2, x, Pa, Pb, state, k)
        v, x, w1, w2 = up["v"][0], up["x"][0], w2, up["w"][0]
        state[(k + 1) & 1] = up["state"][0]
    got = env.unvec(x)
    assert float((got - want["x"]).abs().max()) <= 1e-12 * float(want["x"].abs().max())
    assert float((state[steps & 1][:, mref.PHIBAR] - want["phibar"]).abs().max()) <= 1e-12 * float(B.norm())


# ------------------------------------------------------------------------------------------------ (e)
def test_singular_drift_of_the_restated_iteration():
    """(A - lambda_i I) x = b with b orthogonal to the null vector u_i: from x0 = 0 every iterate stays in the
    complement of u_i in exact arithmetic.  The measured drift |<u_i, x>| / |x| of the float64 restated iteration
    is what DESIGN 3.7 records; the kernels are allowed 10 times `singular_drift()["drift"]`."""
    d = singular_drift()
    assert d["resid"] <= 1e-8 * d["bnorm"]
    assert d["drift"] <= 1e-12, d            # measured: 3.2e-15 (float64)


def singular_case(dtype=torch.float64, n=200, seed=21):
    g = torch.Generator().manual_seed(seed)
    ev = torch.linspace(0.5, 20.0, n, dtype=torch.float64)
    A, Q = mref.hermitian(g, dtype, n, ev)
    lam, U = torch.linalg.eigh(A)
    i = 7
    u = U[:, i]
    b = _rhs(g, dtype, 1, n)[0]
    b = b - u * (u.conj() @ b)
    return A, lam[i], u, b


def singular_drift():
    A, lam, u, b = singular_case()
    n = A.shape[-1]
    As = A - lam * torch.eye(n, dtype=A.dtype)
    stop = 1e-9 * b.norm().reshape(1)
    out = mref.iterate(lambda V: V @ As.T, b.reshape(1, n), stop, 3 * n)
    x = out["x"][0]
    return {"drift": float((u.conj() @ x).abs() / x.norm()), "resid": float((b - As @ x).norm()),
            "bnorm": float(b.norm()), "niter": out["niter"]}


def _restated_meets_the_bar(Afull, B, E, rtol):
    """the restated iteration on (A - E_c I) x_c = b_c, all batch members and columns: criterion of the GPU test"""
    from tests.test_gpu_minres import _reference
    nb, n, nc = B.shape
    rhs = B.transpose(-2, -1).reshape(nb * nc, n)

    def apply(V):
        V = V.reshape(nb, nc, n)
        out = torch.einsum("bij,bcj->bci", Afull, V)
        if E is not None:
            out = out - V * E.reshape(1, nc, 1)
        return out.reshape(nb * nc, n)

    stop = torch.clamp(rtol * rhs.norm(dim=-1), min=1e-8)
    out = mref.iterate(apply, rhs, stop, 4 * n)
    X = out["x"].reshape(nb, nc, n).transpose(-2, -1)
    Xref, kap = _reference(Afull, B, E)
    assert out["niter"] < n / 2, (out["niter"], n)      # geometric convergence, far from exhausting the Krylov space
    assert float((X - Xref).norm()) <= 2 * rtol * kap * float(Xref.norm()), (float((X - Xref).norm() / Xref.norm()), kap)
    h = out["hist"]
    assert all(h[i + 1] <= h[i] for i in range(len(h) - 1))
    return kap


@pytest.mark.parametrize("rtol", [1e-9, 1e-4])
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["real", "complex"])
def test_solver_inputs_meet_the_criterion_on_the_restated_iteration(dtype, rtol):
    from tests import test_gpu_minres as tg
    A, B, _ = tg.dense_input(dtype)
    for E in (None, torch.tensor([0.2, -0.2], dtype=torch.float64)):
        assert _restated_meets_the_bar(A, B, E, rtol) <= 100
    L, sigma, kappa, Bl = tg.laplacian_input(dtype)
    assert kappa <= 100
    _restated_meets_the_bar(L.unsqueeze(0), Bl.unsqueeze(0), torch.full((2,), sigma, dtype=torch.float64), rtol)
    if not dtype.is_complex:
        band, Bb = tg.banded_input(dtype)
        for E in (None, torch.tensor([0.1, -0.2], dtype=torch.float64)):
            assert _restated_meets_the_bar(tg.banded_full(band), Bb, E, rtol) <= 100
