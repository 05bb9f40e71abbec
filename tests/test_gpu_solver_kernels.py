"""-m gpu: the solver-side kernels xk_gmres_step / xk_gmres_finish / xk_gmres_solve (xk_gmres.hip), xk_vec_dots /
xk_broyden_axpy (xk_broyden.hip) and xk_dense_outer / xk_banded_grad (xk_grad.hip), in float64 and float32, against
the reference of tests/solver_ref.py with dtype-derived per-entry bounds.

The kernels are driven through the entry points the drivers use (`_capi.fn("xk_gmres_*")`, `K.vec_dots`,
`K.broyden_axpy`, `K.dense_outer`, `K.banded_grad`) on the configurations of solver_ref (shared with the CPU fault test
tests/test_solver_ref.py).  Every case also checks what must NOT change: all buffers are NaN-poisoned outside the
entries a kernel may write and must come back bit-identical there."""
import math
import numpy as np
import pytest
import torch
from tests import solver_ref as sr
from xitorch_amd import kernels as K
from xitorch_amd._capi import fn, ptr, stream_ptr, suffix

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = sr.DTYPES
IDS = [sr.DNAME[d] for d in DTYPES]
XK_OK, XK_ERR_ARG, XK_ERR_UNSUPPORTED = 0, -1, -2
NAN = math.nan


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _poison(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _dd(cases):
    return [(d, c) for d in DTYPES for c in cases(d)] if callable(cases) else [(d, c) for d in DTYPES for c in cases]


def _ids(pairs):
    return ["%s-%s" % (sr.DNAME[d], "-".join(str(x) for x in c)) for d, c in pairs]


# ================================================================================================ xk_gmres_step
def _step(sfx, c1, c2n, k, cap, R, cs, sn, g, inv, est, S):
    return fn("xk_gmres_step_" + sfx)(ptr(c1), c1.stride(0), ptr(c2n), c2n.stride(0), k, cap, ptr(R), ptr(cs),
                                      ptr(sn), ptr(g), ptr(inv), ptr(est), S, stream_ptr())


STEP = _dd(sr.STEP_CONFIGS)


@pytest.mark.parametrize("dtype,cfg", STEP, ids=_ids(STEP))
def test_gmres_step_single(dev, dtype, cfg):
    """one step on random state: the written entries against the reference, everything else bit-identical (R, cs, sn,
    g are NaN outside what step k reads; est2 is written at pitch 64 only; systems >= S stay untouched)"""
    k, S, edge = cfg
    c = sr.step_case(dtype, k, S, edge)
    Sa, cap = S + sr.STEP_EXTRA_SYSTEMS, c["cap"]
    d = {n: c[n].to(DEV) for n in ("c1", "c2n", "R", "cs", "sn", "g")}
    inv, est = _poison((Sa,), dtype), _poison((Sa, 64), dtype)
    assert _step(suffix(dtype), d["c1"], d["c2n"], k, cap, d["R"], d["cs"], d["sn"], d["g"], inv, est, S) == XK_OK
    torch.cuda.synchronize()
    R, cs, sn, g, inv, est = (t.cpu() for t in (d["R"], d["cs"], d["sn"], d["g"], inv, est))
    got = dict(Rcol=R[:S, :k + 1, k], cs_k=cs[:S, k], sn_k=sn[:S, k], g_k=g[:S, k], g_k1=g[:S, k + 1],
               inv_hn=inv[:S], est2=est[:S, 0])
    what = "gmres_step %s k=%d S=%d %s" % (sr.DNAME[dtype], k, S, edge)
    sr.check(got, sr.step_ref(dtype, c), "gmres_step", dtype, what)
    want = {n: c[n].clone() for n in ("R", "cs", "sn", "g")}
    want["R"][:S, :k + 1, k] = R[:S, :k + 1, k]
    want["cs"][:S, k], want["sn"][:S, k] = cs[:S, k], sn[:S, k]
    want["g"][:S, k:k + 2] = g[:S, k:k + 2]
    for n, t in (("R", R), ("cs", cs), ("sn", sn), ("g", g)):
        assert _same_bits(t, want[n]), "%s: %s changed outside the entries of step k" % (what, n)
    assert bool(torch.isnan(est[:, 1:]).all()) and bool(torch.isnan(est[S:]).all()), what + ": est2 off its pitch"
    assert bool(torch.isnan(inv[S:]).all()), what + ": inv_hn beyond S"
    if edge == "n2_neg":
        assert bool((inv[:S] == 0).all()) and bool((sn[:S, k] == 0).all()) and bool((g[:S, k + 1] == 0).all())
        assert bool((cs[:S, k].abs() == 1).all())
    if edge == "a0_hn0":
        assert bool((cs[:S, k] == 1).all()) and bool((sn[:S, k] == 0).all()) and bool((R[:S, k, k] == 0).all())
        assert bool((inv[:S] == 0).all())
    if edge == "a0_hnpos":
        assert bool((cs[:S, k] == 0).all()) and bool((sn[:S, k] == 1).all())
    if edge == "a_neg":
        assert bool((cs[:S, k] < 0).all()), what + ": the sign of c must follow a"


CHAIN = _dd([(m,) for m in sr.CHAIN_MS])


@pytest.mark.parametrize("dtype,cfg", CHAIN, ids=_ids(CHAIN))
def test_gmres_step_chained(dev, dtype, cfg):
    """m steps from zeroed state: the whole final state step by step against the reference recurrence fed with the
    rotations the kernel stored, and R against the free-running reference (solver_ref.gmres_chain)"""
    m, = cfg
    c = sr.chain_case(dtype, m)
    S, cap = c["S"], c["cap"]
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=DEV)
    R, cs, sn, g = z(S, cap + 1, cap), z(S, cap), z(S, cap), z(S, cap + 1)
    g[:, 0] = c["beta"].to(DEV)
    inv, est = _poison((S,), dtype), _poison((S, 64), dtype)
    for k in range(m):
        assert _step(suffix(dtype), c["c1s"][k].to(DEV), c["c2ns"][k].to(DEV), k, cap, R, cs, sn, g, inv, est, S) == XK_OK
    torch.cuda.synchronize()
    R, cs, sn, g = (t.cpu() for t in (R, cs, sn, g))
    ref = sr.chain_ref(dtype, c, state=dict(cs=cs, sn=sn))
    got = dict(R=R[:, :m + 1, :m], cs=cs[:, :m], sn=sn[:, :m], g=g[:, :m + 1], R_global=R[:, :m + 1, :m])
    sr.check(got, ref, "gmres_step_chain", dtype, "gmres_step chain %s m=%d" % (sr.DNAME[dtype], m))
    assert bool((R[:, m + 1:] == 0).all()) and bool((R[:, :, m:] == 0).all()) and bool((cs[:, m:] == 0).all())
    assert bool((torch.tril(R[:, :m + 1, :m], -1) == 0).all()), "R written below its diagonal"


# ================================================================================================ xk_gmres_solve
SOLVE = _dd(sr.SOLVE_CONFIGS)


@pytest.mark.parametrize("dtype,cfg", SOLVE, ids=_ids(SOLVE))
def test_gmres_solve(dev, dtype, cfg):
    """back substitution with NaN below the diagonal and in columns >= kd (never read), y[kd:] poisoned and untouched,
    y_i = 0 at a zero pivot"""
    kd, S, zero = cfg
    c = sr.solve_case(dtype, kd, S, zero)
    y = _poison((S, c["sy"]), dtype)
    R, g = c["R"].to(DEV), c["g"].to(DEV)
    assert fn("xk_gmres_solve_" + suffix(dtype))(ptr(R), ptr(g), ptr(y), y.stride(0), S, kd, c["cap"],
                                                  stream_ptr()) == XK_OK
    torch.cuda.synchronize()
    y = y.cpu()
    what = "gmres_solve %s kd=%d S=%d zero=%s" % (sr.DNAME[dtype], kd, S, zero)
    sr.check({"y": y[:, :kd]}, sr.solve_ref(dtype, c), "gmres_solve", dtype, what)
    assert bool(torch.isnan(y[:, kd:]).all()), what + ": y written beyond kd"
    assert _same_bits(R, c["R"]) and _same_bits(g, c["g"])
    if zero is not None:
        i = {"last": kd - 1, "first": 0, "mid": kd // 2}[zero]
        assert bool((y[:, i] == 0).all())


# ================================================================================================ xk_gmres_finish
def _finish(sfx, Q, c2n, inv, S, N, k, ldq, sQ):
    return fn("xk_gmres_finish_" + sfx)(ptr(Q), ptr(c2n), c2n.stride(0), ptr(inv), S, N, k, ldq, sQ, stream_ptr())


FINISH = [(d, N) for d in DTYPES for N in sr.finish_ns(d)]


@pytest.mark.parametrize("dtype,N", FINISH, ids=["%s-N%d" % (sr.DNAME[d], N) for d, N in FINISH])
def test_gmres_finish(dev, dtype, N):
    """row k + 1 against the reference ([N, npad) zero in and zero out, an exactly zero row for inv_hn = 0); the whole
    flat allocation is bit-identical elsewhere: rows <= k, the spare row, columns [npad, ldq), the gaps between
    systems"""
    for cfg in sr.finish_configs(dtype):
        if cfg[0] != N:
            continue
        _, k, wide, S = cfg
        c = sr.finish_case(dtype, N, k, wide, S)
        flat = c["flat"].to(DEV)
        assert _finish(suffix(dtype), flat, c["c2n"].to(DEV), c["inv_hn"].to(DEV), S, N, k, c["ldq"], c["sQ"]) == XK_OK
        torch.cuda.synchronize()
        flat = flat.cpu()
        Q = flat.as_strided(c["Q"].shape, c["Q"].stride())
        what = "gmres_finish %s N=%d k=%d ldq=%d S=%d" % (sr.DNAME[dtype], N, k, c["ldq"], S)
        row = Q[:, k + 1, :c["npad"]].clone()
        sr.check({"row": row}, sr.finish_ref(dtype, c), "gmres_finish", dtype, what)
        if S == 3:
            assert bool((row[1] == 0).all()), what + ": breakdown row not zero"
        want = c["flat"].clone()
        want.as_strided(c["Q"].shape, c["Q"].stride())[:, k + 1, :c["npad"]] = row
        assert _same_bits(flat, want), what + ": written outside row k + 1"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_argument_checks(dev, dtype):
    """the C entry points refuse these before anything is launched"""
    sfx, vn = suffix(dtype), sr.VEC_ELEMS[dtype]
    Q = torch.zeros(8 * 64 + vn, dtype=dtype, device=DEV)
    c2n, inv = torch.zeros(8, dtype=dtype, device=DEV), torch.ones(1, dtype=dtype, device=DEV)
    assert _finish(sfx, Q, c2n, inv, 1, 16, 1, 64, 8 * 64) == XK_OK
    assert _finish(sfx, Q, c2n, inv, 1, 16, 1, 64 + 1, 8 * 64) == XK_ERR_UNSUPPORTED       # ldq % VN != 0
    assert _finish(sfx, Q[1:], c2n, inv, 1, 16, 1, 64, 8 * 64) == XK_ERR_UNSUPPORTED       # misaligned Q
    assert _finish(sfx, Q, c2n, inv, 1, 16 + 1, 1, 16, 8 * 64) == XK_ERR_UNSUPPORTED       # ldq < npad
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    t = torch.zeros(64, dtype=dtype, device=DEV)
    for k, cap in ((4, 4), (5, 4)):
        assert _step(sfx, t, t, k, cap, d, d, d, d, t, t, 1) == XK_ERR_ARG                  # k >= cap
    solve = fn("xk_gmres_solve_" + sfx)
    assert solve(ptr(d), ptr(d), ptr(t), 64, 1, 5, 4, stream_ptr()) == XK_ERR_ARG           # kd > cap
    assert solve(ptr(d), ptr(d), ptr(t), 8193, 1, 8193, 8193, stream_ptr()) == XK_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((Q[8 * 64:] == 0).all())


# ================================================================================================ composite Arnoldi
def _rebuild_h(R, cs, sn, m):
    """H = (G_{m-1} ... G_0)^T [R; 0]: the Hessenberg matrix whose rotated form the state holds"""
    H = torch.zeros((m + 1, m), dtype=torch.float64)
    for k in range(m):
        col = torch.zeros(m + 1, dtype=torch.float64)
        col[:k + 1] = R[:k + 1, k]
        for j in range(k, -1, -1):
            p, n = col[j].clone(), col[j + 1].clone()
            col[j], col[j + 1] = cs[j] * p - sn[j] * n, sn[j] * p + cs[j] * n
        H[:, k] = col
    return H


def test_gmres_composite_arnoldi(dev):
    """70 Arnoldi steps of step / finish / solve on a random operator of order 300 in float64, driven like
    native_krylov.gmres (Gram passes with K.dense_mm, first projection with K.lincomb), against a float64 CPU Arnoldi
    with modified Gram-Schmidt twice (MGS2).  This tolerance cannot come from roundoff alone (the Krylov vectors
    depend on the orthogonalisation order): every quantity may differ from MGS2 by 10 times what the CPU Arnoldi with
    classical Gram-Schmidt twice (CGS2) differs from it, with the floor 1e3 u cond(H) (relative to the largest entry).
    Measured on the CPU for this operator (seed 20, both right-hand sides): max |Q_cgs2 - Q_mgs2| = 3.2e-15 / 4.2e-15,
    |H| 1.7e-15 / 2.2e-15, |y| 4.9e-15 / 6.0e-15 (max |y| = 8.6), orthonormality <= 6.7e-16, Arnoldi relation
    <= 6.7e-16, cond(H) = 1.83: the floor 1e3 u cond(H) = 2.0e-13 decides every comparison."""
    N, m, S, ld = 300, 70, 2, 304
    g = torch.Generator().manual_seed(20)
    A = 2 * torch.eye(N, dtype=torch.float64) + 0.5 / math.sqrt(N) * torch.randn(N, N, dtype=torch.float64, generator=g)
    B = torch.randn(S, N, dtype=torch.float64, generator=g)
    Ad = A.to(DEV)
    cap = m + 1
    Q = torch.zeros((S, cap, ld), dtype=torch.float64, device=DEV)
    beta = B.norm(dim=-1)
    Q[:, 0, :N] = (B / beta.unsqueeze(-1)).to(DEV)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=DEV)
    R, cs, sn, gg = z(S, m + 1, m), z(S, m), z(S, m), z(S, m + 1)
    gg[:, 0] = beta.to(DEV)
    inv, est = z(S), z(S, 64)
    for j in range(m):
        wrow = Q[:, j + 1:j + 2]
        K.dense_mm(Ad, Q[:, j:j + 1, :N], out=wrow[:, :, :N])
        c1 = K.dense_mm(Q[:, :j + 1, :N], wrow[:, :, :N])
        K.lincomb(Q, c1, wrow, j + 1, 1, coef_layout="ca", alpha=-1.0, beta=1.0)
        c2n = K.dense_mm(Q[:, :j + 2, :N], wrow[:, :, :N])
        assert _step("f64", c1, c2n, j, m, R, cs, sn, gg, inv, est, S) == XK_OK
        assert _finish("f64", Q, c2n, inv, S, N, j, Q.stride(1), Q.stride(0)) == XK_OK
    y = z(S, 1, cap)
    assert fn("xk_gmres_solve_f64")(ptr(R), ptr(gg), ptr(y), y.stride(0), S, m, m, stream_ptr()) == XK_OK
    torch.cuda.synchronize()
    Q, R, cs, sn, y = (t.cpu() for t in (Q, R, cs, sn, y))
    u = 2.0 ** -53
    eye = torch.eye(m + 1, dtype=torch.float64)
    for s in range(S):
        Qm, Hm = sr.arnoldi(A, B[s], m, "mgs2")
        Qc, Hc = sr.arnoldi(A, B[s], m, "cgs2")
        ym, yc = sr.lstsq_y(Hm, float(beta[s])), sr.lstsq_y(Hc, float(beta[s]))
        floor = 1e3 * u * float(np.linalg.cond(Hm.numpy()))
        Qg, Hg, yg = Q[s, :, :N], _rebuild_h(R[s], cs[s], sn[s], m), y[s, 0, :m].numpy()

        def orth(Qx):
            return float((Qx @ Qx.T - eye).abs().max())

        def arn(Qx, Hx):
            return float((A @ Qx[:m].T - Qx.T @ Hx).abs().max())

        rows = (("Q", float((Qg - Qm).abs().max()), float((Qc - Qm).abs().max()), float(Qm.abs().max())),
                ("H", float((Hg - Hm).abs().max()), float((Hc - Hm).abs().max()), float(Hm.abs().max())),
                ("y", float(np.abs(yg - ym).max()), float(np.abs(yc - ym).max()), float(np.abs(ym).max())),
                ("orthonormality", orth(Qg), max(orth(Qm), orth(Qc)), 1.0),
                ("Arnoldi relation", arn(Qg, Hg), max(arn(Qm, Hm), arn(Qc, Hc)), float(Hm.abs().max())))
        for name, got, cpu, scale in rows:
            tol = max(10 * cpu, floor * scale)
            print("composite s=%d %s: gpu %.3e cpu %.3e tol %.3e" % (s, name, got, cpu, tol))
            assert got <= tol, (s, name, got, cpu, tol)
        assert bool((Q[s, :, N:] == 0).all())


# ================================================================================================ xk_vec_dots
VD = _dd(sr.vd_configs)


def _poison_vd_workspace():
    K.vec_dots([(torch.ones(4, dtype=torch.float64, device=DEV),) * 2])          # creates the stream's workspace
    for ws in K._vd_scratch.values():
        ws.fill_(NAN)


@pytest.mark.parametrize("dtype,cfg", VD, ids=_ids(VD))
def test_vec_dots(dev, dtype, cfg):
    """every pair against the reference with the workspace NaN-poisoned, bit-identical on a second call; L = 0 gives
    exact zeros"""
    L, np_, kind = cfg
    c = sr.vd_case(dtype, L, np_, kind)
    dbufs = [b.to(DEV) for b in c["bufs"]]
    pairs = sr.vd_pairs(c, dbufs)
    if kind == "offset":
        assert pairs[2][0].data_ptr() % 16 != 0 and pairs[0][0].data_ptr() % 16 == 0
    if kind == "equal":
        assert pairs[0][0].data_ptr() != pairs[0][1].data_ptr() and torch.equal(pairs[0][0], pairs[0][1])
    _poison_vd_workspace()
    out = K.vec_dots(pairs).cpu()
    _poison_vd_workspace()
    out2 = K.vec_dots(pairs).cpu()
    what = "vec_dots %s L=%d pairs=%d %s" % (sr.DNAME[dtype], L, len(pairs), kind)
    assert out.dtype == torch.float64 and out.shape == (len(pairs),)
    sr.check({"out": out}, sr.vd_ref(dtype, c), "vec_dots", dtype, what)
    assert _same_bits(out, out2), what + ": not deterministic"
    if L == 0:
        assert bool((out == 0).all())
    for b, d in zip(c["bufs"], dbufs):
        assert _same_bits(b, d)


# ================================================================================================ xk_broyden_axpy
AX = [(d, k) for d in DTYPES for k in sr.AX_KS]


@pytest.mark.parametrize("dtype,k", AX, ids=["%s-k%d" % (sr.DNAME[d], k) for d, k in AX])
def test_broyden_axpy(dev, dtype, k):
    """out on [0, L) against the reference for every presence pattern of u0 / u1 / scale; `out` as a fresh vector, as
    u0, as row k of V (rows < k bit-identical, rows > k and the pitch padding untouched) and offset by one element
    (scalar kernel); the guard elements around `out` stay NaN"""
    vn = sr.VEC_ELEMS[dtype]
    for cfg in sr.ax_configs(dtype):
        if cfg[0] != k:
            continue
        c = sr.ax_case(dtype, *cfg)
        L, mode = c["L"], c["mode"]
        dv = lambda t: None if t is None else t.to(DEV)
        V, u0, u1, coef, scale = dv(c["V"]), dv(c["u0"]), dv(c["u1"]), dv(c["coef"]), dv(c["scale"])
        obuf = _poison((L + 1 + vn,), dtype)
        out = {"plain": obuf[:L], "offset": obuf[1:L + 1], "alias_u0": u0, "row_k": V[k, :L]}[mode]
        if mode == "offset":
            assert L % vn == 0 and out.data_ptr() % 16 != 0
        K.broyden_axpy(out, u0, c["g0"], u1, c["g1"], V=V, coef=coef, scale=scale, k=k, gamma=c["gamma"])
        torch.cuda.synchronize()
        what = "broyden_axpy %s %s" % (sr.DNAME[dtype], cfg)
        sr.check({"out": out.cpu()}, sr.ax_ref(dtype, c), "broyden_axpy", dtype, what)
        wantV = c["V"].clone()
        if mode == "row_k":
            wantV[k, :L] = out.cpu()
        assert _same_bits(V, wantV), what + ": V changed outside the output row"
        if mode in ("plain", "offset"):
            lo = 0 if mode == "plain" else 1
            guard = torch.cat([obuf[:lo], obuf[lo + L:]]).cpu()
            assert bool(torch.isnan(guard).all()), what + ": written outside [0, L)"
        for h, d in ((c["u1"], u1), (c["coef"], coef), (c["scale"], scale)) + (((c["u0"], u0),) if mode != "alias_u0" else ()):
            assert h is None or _same_bits(h, d)
    # k > 0 without a buffer: refused by the entry point before any launch
    o = torch.zeros(8, dtype=dtype, device=DEV)
    rc = fn("xk_broyden_axpy_" + suffix(dtype))(ptr(o), ptr(None), 0.0, ptr(None), 0.0, ptr(None), 0, ptr(None),
                                                 ptr(None), 2, 1.0, 8, stream_ptr())
    assert rc == XK_ERR_ARG


# ================================================================================================ xk_grad.hip
OUTER = [(d, C) for d in DTYPES for C in sr.OUTER_CS]


@pytest.mark.parametrize("dtype,C", OUTER, ids=["%s-C%d" % (sr.DNAME[d], C) for d, C in OUTER])
def test_dense_outer_strided(dev, dtype, C):
    """`out` a view with ldg > N and a batch stride > M ldg of a NaN-poisoned allocation, panels with pitches > M / N
    and NaN beyond: the view entry by entry (accumulate: out0 + U^T W), the allocation bit-identical outside it"""
    for cfg in sr.outer_configs(dtype):
        if cfg[0] != C:
            continue
        _, M, N, B, acc = cfg
        c = sr.outer_case(dtype, *cfg)
        U, W, flat = c["U"].to(DEV), c["W"].to(DEV), c["flat"].to(DEV)
        shape, stride = c["G"].shape, c["G"].stride()
        G = flat[c["off"]:].as_strided(shape, stride)
        assert c["ldg"] > N and c["sG"] > M * c["ldg"]
        K.dense_outer(U[:, :C, :M], W[:, :C, :N], out=G, accumulate=acc)
        torch.cuda.synchronize()
        flat = flat.cpu()
        got = flat[c["off"]:].as_strided(shape, stride).clone()
        what = "dense_outer %s %s" % (sr.DNAME[dtype], cfg)
        sr.check({"G": got}, sr.outer_ref(dtype, c), "dense_outer", dtype, what)
        want = c["flat"].clone()
        want[c["off"]:].as_strided(shape, stride).copy_(got)
        assert _same_bits(flat, want), what + ": written outside the view"


BANDED = [(d, hb) for d in DTYPES for hb in sr.BANDED_HBS]


@pytest.mark.parametrize("dtype,hb", BANDED, ids=["%s-hb%d" % (sr.DNAME[d], hb) for d, hb in BANDED])
def test_banded_grad_edges(dev, dtype, hb):
    """the band gradient entry by entry: entries whose column falls outside the matrix exactly 0 (exactly unchanged
    when accumulating: their bound is 0), C = 0 exact zeros / `out` left alone, the guard zones around `out` NaN"""
    for cfg in sr.banded_configs(dtype):
        if cfg[0] != hb:
            continue
        _, N, C, acc = cfg
        c = sr.banded_case(dtype, *cfg)
        U, W, flat = c["U"].to(DEV), c["W"].to(DEV), c["flat"].to(DEV)
        n = c["G"].numel()
        G = flat[c["off"]:c["off"] + n].view(c["G"].shape)
        K.banded_grad(U[:, :C, :N], W[:, :C, :N], 2 * hb + 1, out=G, accumulate=acc)
        torch.cuda.synchronize()
        flat = flat.cpu()
        got = flat[c["off"]:c["off"] + n].view(c["G"].shape).clone()
        what = "banded_grad %s %s" % (sr.DNAME[dtype], cfg)
        ref = sr.banded_ref(dtype, c)
        sr.check({"G": got}, ref, "banded_grad", dtype, what)
        if C == 0:
            assert _same_bits(got, c["G"] if acc else torch.zeros_like(got)), what
        want = c["flat"].clone()
        want[c["off"]:c["off"] + n] = got.reshape(-1)
        assert _same_bits(flat, want), what + ": written outside out"


def test_report_worst_ratios(dev):
    """the largest |kernel - reference| / bound per kernel and dtype seen by this module's checks (run last)"""
    for key in sorted(sr.WORST):
        print("WORST %s %s: %.3f" % (key[0], key[1], sr.WORST[key]))
    assert all(v <= 1.0 for v in sr.WORST.values())
