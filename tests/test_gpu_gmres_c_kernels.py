"""-m gpu: every entry point of xk_gmres_c.hip (xk_gmres_gram, xk_lincomb, xk_gmres_step, xk_gmres_finish,
xk_gmres_solve; _c128 and _c64) against tests/gmres_c_ref.py within its per-entry bounds, at the configurations
tests/test_gmres_c_ref.py plants its faults at.

Buffers are NaN-poisoned wherever the kernel has no business — the pad [npad, ld) of every vector, basis rows and
coefficient / state entries beyond k, the over-allocated systems of the state, the scratch slots beyond the
S * nblk * (kq + 1) pairs the Gram fold owns — and all of it must come back bit-identical; inputs must not change.  Two
calls of xk_gmres_gram_c* on the same input are bit-identical.  The worst |kernel - value| / bound per (kernel, dtype)
is collected in gmres_c_ref.WORST and printed by the last test."""
import pytest
import torch
from tests import gmres_c_ref as R
from xitorch_amd import kernels as K
from xitorch_amd._capi import fn, ptr, stream_ptr, check, suffix

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), "%s changed" % what


def _ids(cfgs):
    return ["_".join(str(x) for x in c) for c in cfgs]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DNAME[d])
@pytest.mark.parametrize("cfg", R.GRAM_CONFIGS, ids=_ids(R.GRAM_CONFIGS))
def test_gram(dtype, cfg):
    N, kq, S = cfg
    case = R.gram_case(dtype, *cfg)
    Q, w = case["Q"].to(DEV), case["w"].to(DEV)
    c = R.nan_like((S, kq + 1 + R.CAP_EXTRA), dtype).to(DEV)
    need = S * case["nblk"] * (kq + 1) * 2
    scr = torch.full((need + 16,), float("nan"), dtype=torch.float64, device=DEV)
    assert K.gmres_gram_tiles(N, dtype) == case["nblk"]
    K.gmres_gram_c(Q, w, c, scr, kq, N)
    c_first, scr_first = c.clone(), scr.clone()
    K.gmres_gram_c(Q, w, c, scr, kq, N)
    torch.cuda.synchronize()
    _same(c, c_first, "second call: c")
    _same(scr, scr_first, "second call: scratch")
    _same(Q, case["Q"], "Q")
    _same(w, case["w"], "w")
    assert bool(torch.isnan(scr[need:]).all()), "scratch beyond the owned slots written"
    assert bool(torch.isfinite(scr[:need]).all()), "owned scratch slots not all written"
    ch = c.cpu()
    assert bool(torch.isnan(torch.view_as_real(ch[:, kq + 1:])).all()), "c beyond entry kq written"
    got = {"c": ch[:, :kq], "nrm": ch[:, kq].real, "nrm_im": ch[:, kq].imag.double()}
    R.check(got, R.gram_ref(dtype, case), "gram", dtype, what="gram %s %s" % (R.DNAME[dtype], cfg))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DNAME[d])
@pytest.mark.parametrize("cfg", R.LINCOMB_CONFIGS, ids=_ids(R.LINCOMB_CONFIGS))
def test_lincomb(dtype, cfg):
    N, k, S, P, alpha, beta = cfg
    case = R.lincomb_case(dtype, *cfg)
    V, C, out = case["V"].to(DEV), case["C"].to(DEV), case["out0"].clone().to(DEV)
    K.lincomb_c(V, C, out, k, P, alpha=alpha, beta=beta, N=N)
    torch.cuda.synchronize()
    _same(V, case["V"], "V")
    _same(C, case["C"], "C")
    npad = R.npad_of(N, dtype)
    o = out.cpu()
    _same(o[:, P:], case["out0"][:, P:], "output rows beyond P")
    _same(o[:, :, npad:], case["out0"][:, :, npad:], "pad [npad, ld) of the output")
    R.check({"out": o[:, :P, :npad]}, R.lincomb_ref(dtype, case), "lincomb", dtype,
            what="lincomb %s %s" % (R.DNAME[dtype], cfg))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DNAME[d])
@pytest.mark.parametrize("cfg", R.FINISH_CONFIGS, ids=_ids(R.FINISH_CONFIGS))
def test_finish(dtype, cfg):
    N, k, S = cfg
    case = R.finish_case(dtype, *cfg)
    Q, c2n, inv = case["Q"].clone().to(DEV), case["c2n"].to(DEV), case["inv_hn"].to(DEV)
    check(fn("xk_gmres_finish_" + suffix(dtype))(ptr(Q), ptr(c2n), c2n.stride(0), ptr(inv), S, N, k, Q.stride(1),
                                                 Q.stride(0), stream_ptr()), "xk_gmres_finish")
    torch.cuda.synchronize()
    _same(c2n, case["c2n"], "c2n")
    _same(inv, case["inv_hn"], "inv_hn")
    npad = R.npad_of(N, dtype)
    q = Q.cpu()
    _same(q[:, :k + 1], case["Q"][:, :k + 1], "basis rows 0..k")
    _same(q[:, k + 2:], case["Q"][:, k + 2:], "basis rows beyond k+1")
    _same(q[:, k + 1, npad:], case["Q"][:, k + 1, npad:], "pad [npad, ld) of row k+1")
    R.check({"row": q[:, k + 1, :npad]}, R.finish_ref(dtype, case), "finish", dtype,
            what="finish %s %s" % (R.DNAME[dtype], cfg))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DNAME[d])
@pytest.mark.parametrize("cfg", R.STEP_CONFIGS, ids=_ids(R.STEP_CONFIGS))
def test_step(dtype, cfg):
    k, S, edge = cfg
    cap = R.STEP_CAP
    case = R.step_case(dtype, *cfg)
    rdt = R.RDT[dtype]
    c1, c2n = case["c1"].to(DEV), case["c2n"].to(DEV)
    Rm, cs, sn, g = (case[n].clone().to(DEV) for n in ("R", "cs", "sn", "g"))
    inv = torch.full((S + 1,), float("nan"), dtype=rdt, device=DEV)
    est = torch.full((S + 1, 64), float("nan"), dtype=rdt, device=DEV)
    check(fn("xk_gmres_step_" + suffix(dtype))(ptr(c1), c1.stride(0), ptr(c2n), c2n.stride(0), k, cap, ptr(Rm), ptr(cs),
                                               ptr(sn), ptr(g), ptr(inv), ptr(est), S, stream_ptr()), "xk_gmres_step")
    torch.cuda.synchronize()
    _same(c1, case["c1"], "c1")
    _same(c2n, case["c2n"], "c2n")
    Rc, csc, snc, gc, invc, estc = Rm.cpu(), cs.cpu(), sn.cpu(), g.cpu(), inv.cpu(), est.cpu()
    # only column k of R (rows 0..k), cs[k], sn[k], g[k], g[k+1] of the first S systems may change
    Rexp, csexp, snexp, gexp = case["R"].clone(), case["cs"].clone(), case["sn"].clone(), case["g"].clone()
    Rexp[:S, :k + 1, k] = Rc[:S, :k + 1, k]
    csexp[:S, k], snexp[:S, k] = csc[:S, k], snc[:S, k]
    gexp[:S, k:k + 2] = gc[:S, k:k + 2]
    _same(Rc, Rexp, "R outside column k")
    _same(csc, csexp, "cs outside entry k")
    _same(snc, snexp, "sn outside entry k")
    _same(gc, gexp, "g outside entries k, k+1")
    assert bool(torch.isnan(invc[S:]).all()) and bool(torch.isnan(estc[S:]).all()) and \
        bool(torch.isnan(estc[:S, 1:]).all()), "inv_hn / est2 written outside their slots"
    got = {"Rcol": Rc[:S, :k + 1, k], "cs_k": csc[:S, k], "sn_k": snc[:S, k], "g_k": gc[:S, k], "g_k1": gc[:S, k + 1],
           "inv_hn": invc[:S], "est2": estc[:S, 0]}
    R.check(got, R.step_ref(dtype, case), "step", dtype, what="step %s %s" % (R.DNAME[dtype], cfg))
    if edge == "a0":
        assert bool((csc[:S, k] == 0).all()) and bool((snc[:S, k] == 1).all()), "a = 0 must give cs = 0, sn = 1"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DNAME[d])
@pytest.mark.parametrize("cfg", R.SOLVE_CONFIGS, ids=_ids(R.SOLVE_CONFIGS))
def test_solve(dtype, cfg):
    kd, S, zero = cfg
    case = R.solve_case(dtype, *cfg)
    Rm, g = case["R"].to(DEV), case["g"].to(DEV)
    y0 = R.nan_like((S, kd + 3), dtype)
    y = y0.clone().to(DEV)
    check(fn("xk_gmres_solve_" + suffix(dtype))(ptr(Rm), ptr(g), ptr(y), y.stride(0), S, kd, case["cap"],
                                                stream_ptr()), "xk_gmres_solve")
    torch.cuda.synchronize()
    _same(Rm, case["R"], "R")
    _same(g, case["g"], "g")
    yc = y.cpu()
    _same(yc[:, kd:], y0[:, kd:], "y beyond kd")
    R.check({"y": yc[:, :kd]}, R.solve_ref(dtype, case), "solve", dtype, what="solve %s %s" % (R.DNAME[dtype], cfg))
    if zero is not None:
        assert bool((yc[:, zero] == 0).all())


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DNAME[d])
def test_argument_checks(dtype):
    sfx = suffix(dtype)
    z = torch.zeros(64, dtype=dtype, device=DEV)
    zr = torch.zeros(64, dtype=torch.float64, device=DEV)
    # the back substitution keeps y in LDS: 16 B per entry, kd <= 4096
    assert fn("xk_gmres_solve_" + sfx)(ptr(zr), ptr(zr), ptr(z), 8192, 1, 4097, 8192, stream_ptr()) == -2
    # nblk must be the tile count of N
    assert fn("xk_gmres_gram_" + sfx)(ptr(z), ptr(z), ptr(z), ptr(zr), 1, 8, 0, 8, 8, 8, 8, 2, stream_ptr()) == -1
    # complex64: an odd pitch breaks the 16 B alignment of the rows
    if dtype == torch.complex64:
        assert fn("xk_gmres_finish_" + sfx)(ptr(z), ptr(z), 8, ptr(zr), 1, 4, 0, 5, 16, stream_ptr()) == -2
    # an empty vector: no tile (nblk = 0), the sums are empty and c[s, 0..kq] = 0
    c = R.nan_like((2, 4), dtype).to(DEV)
    assert fn("xk_gmres_gram_" + sfx)(ptr(z), ptr(z), ptr(c), ptr(zr), 2, 0, 2, 8, 8, 8, 4, 0, stream_ptr()) == 0
    torch.cuda.synchronize()
    cc = c.cpu()
    assert bool((cc[:, :3] == 0).all()) and bool(torch.isnan(torch.view_as_real(cc[:, 3:])).all())


def test_zz_report_worst_ratios():
    """prints the worst |kernel - value| / bound per (kernel, dtype) of this session (run with -s to see it)"""
    for key in sorted(R.WORST):
        print("gmres_c worst |err|/bound %-8s %-5s %.3f" % (key[0], key[1], R.WORST[key]))
        assert R.WORST[key] <= 1.0
