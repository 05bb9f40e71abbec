"""CPU: the reference of tests/solver_ref.py (GMRES state kernels, Broyden BLAS-1, operator gradients) agrees with
independent formulations, its checker accepts a correct output rounded to the kernel dtype, and it rejects every fault
of solver_ref.FAULTS_* at EVERY configuration of tests/test_gpu_solver_kernels.py where solver_ref.VISIBLE says the
fault can show -- and every fault shows in at least one of them, so the configuration lists cannot shrink into
blindness."""
import math
import numpy as np
import pytest
import torch
from tests import solver_ref as sr

DTYPES = sr.DTYPES
IDS = [sr.DNAME[d] for d in DTYPES]
LD = np.longdouble


def _rejected(got, ref, kernel, dtype):
    try:
        sr.check(got, ref, kernel, dtype)
    except AssertionError:
        return True
    return False


def _sweep(kernel, dtype, faults, configs, make_ref, visible_args=lambda cfg, ref_case: cfg, keep64=()):
    """at every configuration: the rounded reference is accepted, every visible fault rejected; returns how often each
    fault was visible.  make_ref(cfg) -> (case, ref function of the fault)"""
    seen = {f: 0 for f in faults}
    for cfg in configs:
        case, ref_of = make_ref(cfg)
        ref = ref_of(None)
        assert sr.check(sr.values(ref, dtype, keep64), ref, kernel, dtype, what=str(cfg)) <= 1.0
        for f in faults:
            if sr.VISIBLE[(kernel, f)](*visible_args(cfg, case)):
                seen[f] += 1
                assert _rejected(sr.values(ref_of(f), dtype, keep64), ref, kernel, dtype), \
                    "%s %s: fault %s not rejected at %s" % (kernel, sr.DNAME[dtype], f, cfg)
    for f in faults:
        assert seen[f] >= 1, "fault %s of %s shows at no configuration" % (f, kernel)
    return seen


# ================================================================================================ (a) independent forms
@pytest.mark.parametrize("m", sr.CHAIN_MS)
def test_gmres_chain_and_solve_reproduce_lstsq_and_qr(m):
    """the chained step reference followed by the reference back substitution gives numpy.linalg.lstsq(H, beta e1)
    (1e-13 relative to max |y|), its R is the R factor of numpy.linalg.qr(H) with a positive diagonal, and |g[m]| is
    the least-squares residual: against lstsq's explicit residual for m <= 5 only (1e-12 relative); beyond, |g[m]|
    keeps shrinking geometrically below what any explicit residual can resolve, so there the explicit residual of the
    reference's y, formed in numpy.longdouble, must merely not exceed |g[m]| + 1e-14 beta"""
    dtype = torch.float64
    c = sr.chain_case(dtype, m)
    free = sr.chain_ref(dtype, c)
    H = sr.hessenberg_of(c["c1s"], c["c2ns"])
    y = sr.gmres_solve(dtype, free["R"][0], free["g"][0], m)["y"][0].numpy()
    for s in range(c["S"]):
        H64, beta = np.asarray(H[s], dtype=np.float64), float(c["beta"][s])
        yl = sr.lstsq_y(H64, beta)
        assert np.abs(y[s] - yl).max() <= 1e-13 * np.abs(yl).max()
        q, r = np.linalg.qr(H64)
        r = r * np.sign(np.diag(r))[:, None]
        cond = np.linalg.cond(H64)
        assert np.abs(free["R"][0][s, :m].numpy() - r).max() <= 1e-14 * m * cond * np.abs(r).max()
        rhs = np.zeros(m + 1, LD)
        rhs[0] = beta
        res = float(np.sqrt(((rhs - H[s] @ y[s].astype(LD)) ** 2).sum()))
        gm = abs(float(free["g"][0][s, m]))
        assert res <= gm + 1e-14 * beta
        if m <= 5:
            resl = float(np.linalg.norm(rhs.astype(np.float64) - H64 @ yl))
            assert abs(gm - resl) <= 1e-12 * resl


def test_gmres_step_agrees_with_a_dense_rotation_product():
    """one step = the stored rotations as explicit 2 x 2 blocks applied to the column [c1 + c2; hn], then the rotation
    that annihilates its last entry"""
    dtype = torch.float64
    for k in (0, 1, 2, 31):
        c = sr.step_case(dtype, k, 3, None)
        ref = sr.step_ref(dtype, c)
        for s in range(3):
            col = np.zeros(k + 2)
            col[:k + 1] = (c["c1"][s, :k + 1] + c["c2n"][s, :k + 1]).numpy()
            col[k + 1] = math.sqrt(float(c["c2n"][s, k + 1] - (c["c2n"][s, :k + 1] ** 2).sum()))
            for j in range(k):
                G = np.eye(k + 2)
                cj, tj = float(c["cs"][s, j]), float(c["sn"][s, j])
                G[j:j + 2, j:j + 2] = [[cj, tj], [-tj, cj]]
                col = G @ col
            den = math.hypot(col[k], col[k + 1])
            assert abs(float(ref["cs_k"][0][s]) - col[k] / den) <= 1e-13
            assert abs(float(ref["sn_k"][0][s]) - col[k + 1] / den) <= 1e-13
            want = np.append(col[:k], den)
            assert np.abs(ref["Rcol"][0][s].numpy() - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
            gk = float(c["g"][s, k])
            assert abs(float(ref["g_k1"][0][s]) + col[k + 1] / den * gk) <= 1e-13
            assert abs(float(ref["est2"][0][s]) - (col[k + 1] / den * gk) ** 2) <= 1e-13
            assert abs(float(ref["inv_hn"][0][s]) * col[k + 1] - 1) <= 1e-12 if k == 0 else True


def test_gmres_solve_and_finish_agree_with_numpy():
    dtype = torch.float64
    c = sr.solve_case(dtype, 65, 3, None)
    y = sr.solve_ref(dtype, c)["y"][0]
    for s in range(3):
        R = np.triu(np.nan_to_num(c["R"][s, :65, :65].numpy()))
        yn = np.linalg.solve(R, c["g"][s, :65].numpy())
        assert np.abs(y[s].numpy() - yn).max() <= 1e-12 * np.abs(yn).max()
    c = sr.finish_case(dtype, 37, 5, 3, 3)
    row = sr.finish_ref(dtype, c)["row"][0]
    for s in range(3):
        w = c["Q"][s, 6, :38].clone()
        for j in range(6):
            w = w - c["c2n"][s, j] * c["Q"][s, j, :38]
        assert float((row[s] - w * c["inv_hn"][s]).abs().max()) <= 1e-14
    assert bool((row[1] == 0).all()) and bool((row[:, 37:] == 0).all())


def test_blas1_references_agree_with_exact_and_looped_sums():
    for dtype in DTYPES:
        c = sr.vd_case(dtype, 8193, 4, "plain")
        out = sr.vd_ref(dtype, c)["out"][0]
        for i, (a, b) in enumerate(sr.vd_pairs(c)):
            exact = math.fsum(x * y for x, y in zip(a.double().tolist(), b.double().tolist()))
            assert abs(float(out[i]) - exact) <= 1e-15 * 8193 * sr.HUGE ** 2
        cfg = (5, 7, 4096, 8, "plain", 17)
        c = sr.ax_case(dtype, *cfg)
        ref = sr.ax_ref(dtype, c)["out"][0]
        g0, g1, gm = (sr.cast(c[n], dtype) for n in ("g0", "g1", "gamma"))
        acc = torch.zeros(4096, dtype=torch.float64)
        for n in range(5):
            acc += float((c["coef"][n] * c["scale"][n])) * c["V"][n, :4096].double()
        want = g0 * c["u0"].double() + g1 * c["u1"].double() + gm * acc
        assert float((ref - want).abs().max()) <= 1e-13
    assert sr.vd_layout(0) == (8192, 1) and sr.vd_layout(8192 * 1024) == (8192, 1024)
    assert sr.vd_layout(8192 * 1024 + 1) == (8448, 993)


def test_banded_reference_is_the_band_of_the_dense_outer_product():
    dtype = torch.float64
    for hb, N, C in ((0, 7, 3), (5, 5, 9), (5, 6, 1), (63, 200, 17)):
        c = sr.banded_case(dtype, hb, N, C, False)
        U, W = c["U"][:, :C, :N], c["W"][:, :C, :N]
        G = sr.banded_grad(dtype, U, W, hb)["G"][0]
        D = sr.dense_outer(dtype, U, W)["G"][0]
        for d in range(2 * hb + 1):
            for i in range(N):
                j = i + d - hb
                want = D[:, i, j] if 0 <= j < N else torch.zeros(c["B"], dtype=torch.float64)
                assert float((G[:, d, i] - want).abs().max()) <= 1e-13


# ================================================================================================ (b) faults
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_step_faults_rejected_everywhere(dtype):
    def make(cfg):
        c = sr.step_case(dtype, *cfg)
        return c, lambda f: sr.step_ref(dtype, c, f)
    _sweep("step", dtype, sr.FAULTS_GMRES_STEP, sr.STEP_CONFIGS, make, keep64=sr.STEP_STATE)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_chain_faults_rejected_everywhere(dtype):
    """as the GPU test does: the state a (faulty) kernel left behind against the recurrence replayed with the
    rotations found in that state"""
    faults = [f for (kern, f) in sr.VISIBLE if kern == "chain"]
    seen = {f: 0 for f in faults}
    for m in sr.CHAIN_MS:
        c = sr.chain_case(dtype, m)
        for f in [None] + faults:
            out = sr.chain_ref(dtype, c, None, f)
            got = {n: out[n][0] for n in ("R", "cs", "sn", "g")}
            got["R_global"] = got["R"]
            ref = sr.chain_ref(dtype, c, dict(cs=got["cs"], sn=got["sn"]))
            if f is None:
                assert sr.check(got, ref, "chain", dtype) <= 1.0
            elif sr.VISIBLE[("chain", f)](m):
                seen[f] += 1
                assert _rejected(got, ref, "chain", dtype), "chain m=%d: %s not rejected" % (m, f)
    assert all(v >= 1 for v in seen.values()), seen


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_solve_faults_rejected_everywhere(dtype):
    def make(cfg):
        c = sr.solve_case(dtype, *cfg)
        return c, lambda f: sr.solve_ref(dtype, c, f)
    _sweep("solve", dtype, sr.FAULTS_GMRES_SOLVE, sr.SOLVE_CONFIGS, make)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_finish_faults_rejected_everywhere(dtype):
    def make(cfg):
        c = sr.finish_case(dtype, *cfg)
        return c, lambda f: sr.finish_ref(dtype, c, f)
    _sweep("finish", dtype, sr.FAULTS_GMRES_FINISH, sr.finish_configs(dtype), make)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vec_dots_faults_rejected_everywhere(dtype):
    vn = sr.VEC_ELEMS[dtype]

    def make(cfg):
        c = sr.vd_case(dtype, *cfg)
        return c, lambda f: sr.vd_ref(dtype, c, f)
    _sweep("vec_dots", dtype, sr.FAULTS_VEC_DOTS, sr.vd_configs(dtype), make,
           visible_args=lambda cfg, c: cfg + (vn,), keep64=("out",))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_broyden_axpy_faults_rejected_everywhere(dtype):
    def make(cfg):
        c = sr.ax_case(dtype, *cfg)
        return c, lambda f: sr.ax_ref(dtype, c, f)
    _sweep("axpy", dtype, sr.FAULTS_AXPY, sr.ax_configs(dtype), make, visible_args=lambda cfg, c: (c,))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grad_faults_rejected_everywhere(dtype):
    def make_outer(cfg):
        c = sr.outer_case(dtype, *cfg)
        return c, lambda f: sr.outer_ref(dtype, c, f)

    def make_banded(cfg):
        c = sr.banded_case(dtype, *cfg)
        return c, lambda f: sr.banded_ref(dtype, c, f)
    _sweep("outer", dtype, sr.FAULTS_OUTER, sr.outer_configs(dtype), make_outer)
    _sweep("banded", dtype, sr.FAULTS_BANDED, sr.banded_configs(dtype), make_banded)


def test_every_listed_fault_has_a_visibility_rule():
    want = {("step", f) for f in sr.FAULTS_GMRES_STEP} | {("solve", f) for f in sr.FAULTS_GMRES_SOLVE} | \
           {("finish", f) for f in sr.FAULTS_GMRES_FINISH} | {("vec_dots", f) for f in sr.FAULTS_VEC_DOTS} | \
           {("axpy", f) for f in sr.FAULTS_AXPY} | {("outer", f) for f in sr.FAULTS_OUTER} | \
           {("banded", f) for f in sr.FAULTS_BANDED}
    assert want <= set(sr.VISIBLE)
