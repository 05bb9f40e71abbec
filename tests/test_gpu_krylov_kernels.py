"""-m gpu: every fused Krylov step kernel of xk_krylov.hip (kry_dots, bicg_p, bicg_s, bicg_final, kry_resid,
cg_update, cg_p, kry_status), in all four dtypes, against the float64 / complex128 reference of
tests/krylov_ref.py with dtype-derived bounds.

The kernels are driven through native_krylov._Kry, built from a stub problem; `kr.nblk` is then forced to cover the
multi-block two-stage reductions (block partials + re-reduction), the 64-block cap, and more blocks than 16 B
vectors.  Every case also checks the panel contract: [N, npad) zero in and zero out, [npad, ld) NaN-poisoned and
untouched, partial slots [nblk, 64) NaN-poisoned and ignored by consumers / untouched by producers, and skip_r
leaving r and its partials alone."""
import math
import pytest
import torch
from tests import krylov_ref as kref
from xitorch_amd.linalg import native_krylov as nk
from xitorch_amd.linalg._panel import pad_len

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
EPS = 1e-12
DEV = torch.device("cuda:0")


class _Stub:
    """what _Kry reads of a native_krylov._Problem"""

    def __init__(self, dtype, S, N, ld):
        self.S, self.N, self.ld, self.dtype = S, N, ld, dtype
        self.rdtype = kref.REAL_OF[dtype]
        self.cplx = dtype.is_complex
        self.device = DEV
        self.E = None
        self.vec_elems = kref.VEC_ELEMS[dtype]

    def nblk(self):
        return nk._Problem.nblk(self)           # the driver's own sizing rule


def _configs(dtype):
    """(N, S, extra pitch, forced nblk or None = what _Problem.nblk() picks)"""
    vn = kref.VEC_ELEMS[dtype]
    one = 1024 * vn                  # the largest N that _Problem.nblk() serves with one block
    cfg = [(1, 3, 0, None), (1, 257, 8, None), (vn + 1, 3, 0, None), (5, 3, 8, 7), (1000, 3, 0, None),
           (1000, 257, 8, 2), (1000, 3, 0, 1), (1000, 3, 8, 64), (one, 3, 0, None), (one + 1, 3, 8, None),
           (5 * one + 37, 3, 0, None), (5 * one + 37, 3, 8, 7), (64 * one + 1, 1, 0, None), (300001, 3, 8, None),
           (300001, 1, 0, 2)]
    if vn > 1:
        cfg.insert(1, (vn - 1, 3, 8, None))
    return cfg


CASES = [(d, c) for d in DTYPES for c in _configs(d)]
CASE_IDS = ["%s-N%d-S%d-ld+%d-nb%s" % (IDS[DTYPES.index(d)], c[0], c[1], c[2], c[3]) for d, c in CASES]


class _Case:
    def __init__(self, dtype, N, S, extra, nblk, seed):
        self.dtype, self.N, self.S = dtype, N, S
        self.ld = pad_len(N) + extra
        self.vn = kref.VEC_ELEMS[dtype]
        self.npad = (N + self.vn - 1) // self.vn * self.vn
        self.kr = nk._Kry(_Stub(dtype, S, N, self.ld))
        if nblk is not None:
            self.kr.nblk = nblk
        self.nblk = self.kr.nblk
        self.ctx = kref.Ctx(dtype, S, N, self.nblk, EPS)
        self.g = torch.Generator().manual_seed(seed)
        self.dev = DEV
        self.zero_sys = [s for s in range(S) if s % 3 == 1]           # exactly zero denominators
        self.zero_omega = [s for s in range(S) if s % 4 == 2]

    def vecs(self, n):
        """n (host, device) pairs of contract-shaped (S, ld) arrays"""
        hs = kref.rand_vecs(self.g, self.dtype, self.S, self.N, self.ld, count=n)
        return [(h, h.to(self.dev)) for h in hs]

    def out_vec(self):
        return torch.full((self.S, self.ld), kref.nan_of(self.dtype), dtype=self.dtype, device=self.dev)

    def scalars(self, zero=()):
        h = kref.rand_scalars(self.g, self.dtype, self.S)
        h[list(zero)] = 0
        return h, h.to(self.dev)

    def out_scalar(self):
        return torch.full((self.S,), kref.nan_of(self.dtype), dtype=self.dtype, device=self.dev)

    def partials(self, zero=()):
        h = kref.rand_partials(self.g, self.dtype, self.S, self.nblk, zero_systems=zero)
        return h, h.to(self.dev)

    def out_partials(self, real=False):
        return kref.poisoned_partials(self.dtype, self.S, real=real).to(self.dev)

    # ---- contract checks of kernel outputs; each returns the value the reference is compared with
    def vec(self, t, what):
        t = t.cpu()
        assert bool((t[:, self.N:self.npad] == 0).all()), "%s: [N, npad) not zero" % what
        assert bool(torch.isnan(t[:, self.npad:]).all()), "%s: [npad, ld) written" % what
        return t[:, :self.N]

    def psum(self, P, what):
        P = P.cpu()
        assert bool(torch.isnan(P[:, self.nblk:]).all()), "%s: partial slots [nblk, 64) written" % what
        assert bool(torch.isfinite(P[:, :self.nblk]).all()), "%s: a used partial slot is not finite" % what
        return kref.partial_value(P, self.ctx)[:, :self.nblk].sum(-1)

    def untouched(self, t, what):
        assert bool(torch.isnan(t.cpu()).all()), "%s: written although it must be left alone" % what

    def check(self, got, ref, what):
        return kref.check(got, ref, self.dtype, what="%s [%s N=%d S=%d ld=%d nblk=%d]"
                          % (what, self.dtype, self.N, self.S, self.ld, self.nblk))


def _run_kry_dots(c):
    kr, ctx = c.kr, c.ctx
    (x1h, x1), (y1h, y1), (x2h, x2), (y2h, y2), (zh, z) = c.vecs(5)
    Eh, E = c.scalars()
    X = ctx.vec
    # a) one product
    P1 = c.out_partials()
    kr.dots(x1, y1, P1)
    c.check({"P1": c.psum(P1, "P1")}, kref.kry_dots(ctx, X(x1h), X(y1h)), "kry_dots")
    # b) two independent products
    P1, P2 = c.out_partials(), c.out_partials()
    kr.dots(x1, y1, P1, x2, y2, P2)
    c.check({"P1": c.psum(P1, "P1"), "P2": c.psum(P2, "P2")}, kref.kry_dots(ctx, X(x1h), X(y1h), X(x2h), X(y2h)),
            "kry_dots 2")
    kr.E = E
    # c) the shift of _Problem._shift_now: y1 -= E z with x1 == y1
    yy = y1.clone()
    P1 = c.out_partials()
    kr.dots(yy, yy, P1, shift=z)
    ref = kref.kry_dots(ctx, X(y1h), X(y1h), shiftz=X(zh), E=kref.hp(Eh), x1_is_y1=True)
    c.check({"P1": c.psum(P1, "P1"), "y1": c.vec(yy, "y1")}, ref, "kry_dots shift x1==y1")
    # d) CG: <p, Ap - E z>
    yy = y1.clone()
    P1 = c.out_partials()
    kr.dots(x1, yy, P1, shift=z)
    ref = kref.kry_dots(ctx, X(x1h), X(y1h), shiftz=X(zh), E=kref.hp(Eh))
    c.check({"P1": c.psum(P1, "P1"), "y1": c.vec(yy, "y1")}, ref, "kry_dots shift")
    # e) BiCGStab: <t, s> (conj1) and <t, t>, t = y1 shifted, x2 == y2 == y1
    yy = y1.clone()
    P1, P2 = c.out_partials(), c.out_partials()
    kr.dots(x1, yy, P1, yy, yy, P2, shift=z, conj1=True)
    ref = kref.kry_dots(ctx, X(x1h), X(y1h), shiftz=X(zh), E=kref.hp(Eh), conj1=True,
                        x2_is_y1=True, y2_is_y1=True)
    c.check({"P1": c.psum(P1, "P1"), "P2": c.psum(P2, "P2"), "y1": c.vec(yy, "y1")}, ref, "kry_dots bicg")
    kr.E = None


def _run_bicg_p(c):
    kr, ctx, X = c.kr, c.ctx, c.ctx.vec
    (rh, r), (ph, p), (vh, v) = c.vecs(3)
    Ph, P = c.partials()
    (roh, ro), (ah, a), (omh, om) = c.scalars(c.zero_sys), c.scalars(), c.scalars(c.zero_omega)
    for first in (False, True):
        pp, rs = p.clone(), c.out_scalar()
        kr.bicg_p(r, pp, v, P, ro, a, om, rs, EPS, first)
        ref = kref.bicg_p(ctx, X(rh), X(ph), X(vh), Ph, kref.hp(roh), kref.hp(ah), kref.hp(omh), first)
        c.check({"p": c.vec(pp, "p"), "rho_store": rs.cpu()}, ref, "bicg_p first=%d" % first)


def _run_bicg_s(c):
    kr, ctx, X = c.kr, c.ctx, c.ctx.vec
    (rh, r), (vh, v) = c.vecs(2)
    Ph, P = c.partials(c.zero_sys)
    rhoh, rho = c.scalars()
    s, al = c.out_vec(), c.out_scalar()
    kr.bicg_s(r, v, s, rho, P, al, EPS)
    c.check({"s": c.vec(s, "s"), "alpha_store": al.cpu()}, kref.bicg_s(ctx, X(rh), X(vh), kref.hp(rhoh), Ph), "bicg_s")


def _run_bicg_final(c):
    kr, ctx, X = c.kr, c.ctx, c.ctx.vec
    (xh, x), (yh, y), (zh, z), (sh, s), (th, t), (r0h, r0) = c.vecs(6)
    Ptsh, Pts = c.partials()
    Ptth, Ptt = c.partials(c.zero_sys)
    alh, al = c.scalars()
    for alias, skip in ((True, False), (False, False), (True, True)):
        sv = z if alias else s
        svh = zh if alias else sh
        xo, om, Prr, Prho = c.out_vec(), c.out_scalar(), c.out_partials(real=True), c.out_partials()
        r = c.out_vec()
        if not skip:
            r[:, :c.npad] = 7                  # overwritten on [0, npad)
        kr.bicg_final(x, xo, y, z, sv, t, r, r0, al, Pts, Ptt, om, Prr, Prho, EPS, skip)
        ref = kref.bicg_final(ctx, X(xh), X(yh), X(zh), X(svh), X(th), X(r0h), kref.hp(alh), Ptsh, Ptth, skip)
        got = {"xout": c.vec(xo, "xout"), "omega_store": om.cpu()}
        what = "bicg_final alias=%d skip_r=%d" % (alias, skip)
        if skip:
            for name, buf in (("r", r), ("Prr", Prr), ("Prho", Prho)):
                c.untouched(buf, what + " " + name)
        else:
            got.update(r=c.vec(r, "r"), Prr=c.psum(Prr, "Prr"), Prho=c.psum(Prho, "Prho"))
        c.check(got, ref, what)


def _run_kry_resid(c):
    kr, ctx, X = c.kr, c.ctx, c.ctx.vec
    (bh, b), (yh, y), (r0h, r0) = c.vecs(3)
    for use_r0, use_prho in ((True, True), (False, True), (False, False)):
        r, Prr = c.out_vec(), c.out_partials(real=True)
        Prho = c.out_partials() if use_prho else None
        kr.resid(b, y, r, r0 if use_r0 else None, Prr, Prho)
        got = {"r": c.vec(r, "r"), "Prr": c.psum(Prr, "Prr")}
        if use_prho:
            got["Prho"] = c.psum(Prho, "Prho")
        ref = kref.kry_resid(ctx, X(bh), X(yh), X(r0h) if use_r0 else None, use_prho)
        c.check(got, ref, "kry_resid r0=%d Prho=%d" % (use_r0, use_prho))
    # the drivers' initial residual: partials of b itself (y = a zero panel)
    Prr, Prho = c.out_partials(real=True), c.out_partials()
    kr.resid(b, None, None, r0, Prr, Prho, init=True)
    ref = kref.kry_resid(ctx, X(bh), X(bh) * 0, X(r0h), True)
    del ref["r"]
    c.check({"Prr": c.psum(Prr, "Prr"), "Prho": c.psum(Prho, "Prho")}, ref, "kry_resid init")


def _run_cg_update(c):
    kr, ctx, X = c.kr, c.ctx, c.ctx.vec
    (xh, x), (ph, p), (aph, ap), (rh, r) = c.vecs(4)
    Przh, Prz = c.partials()
    Papph, Papp = c.partials(c.zero_sys)
    for skip in (False, True):
        xo, Prr = c.out_vec(), c.out_partials(real=True)
        rr = c.out_vec() if skip else r.clone()
        kr.cg_update(x, xo, p, ap, rr, Prz, Papp, Prr, EPS, skip)
        ref = kref.cg_update(ctx, X(xh), X(ph), X(aph), X(rh), Przh, Papph, skip)
        got = {"xout": c.vec(xo, "xout")}
        what = "cg_update skip_r=%d" % skip
        if skip:
            c.untouched(rr, what + " r")
            c.untouched(Prr, what + " Prr")
        else:
            got.update(r=c.vec(rr, "r"), Prr=c.psum(Prr, "Prr"))
        c.check(got, ref, what)


def _run_cg_p(c):
    kr, ctx, X = c.kr, c.ctx, c.ctx.vec
    (zh, z), (ph, p) = c.vecs(2)
    Pnh, Pn = c.partials()
    Poh, Po = c.partials(c.zero_sys)
    pp = p.clone()
    kr.cg_p(z, pp, Pn, Po, EPS)
    c.check({"p": c.vec(pp, "p")}, kref.cg_p(ctx, X(zh), X(ph), Pnh, Poh), "cg_p")


RUNNERS = [_run_kry_dots, _run_bicg_p, _run_bicg_s, _run_bicg_final, _run_kry_resid, _run_cg_update, _run_cg_p]


@pytest.mark.parametrize("dtype,cfg", CASES, ids=CASE_IDS)
def test_step_kernels_vs_reference(dev, dtype, cfg):
    N, S, extra, nblk = cfg
    for i, run in enumerate(RUNNERS):
        run(_Case(dtype, N, S, extra, nblk, seed=1000 * i + N % 997 + S))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_counts_agree_and_launches_are_deterministic(dev, dtype):
    """the totals of one product for nblk in {default, 1, 2, 7, 64} agree within the sum of their bounds, and two
    launches on identical inputs write bit-identical partials / vectors (the header's deterministic reductions)"""
    vn = kref.VEC_ELEMS[dtype]
    N, S = 5 * 1024 * vn + 37, 3
    totals = []
    for nblk in (None, 1, 2, 7, 64):
        c = _Case(dtype, N, S, 0, nblk, seed=77)        # same seed: same inputs for every block count
        (x1h, x1), (y1h, y1), (zh, z), (rh, r), (r0h, r0) = c.vecs(5)
        Eh, E = c.scalars()
        c.kr.E = E
        outs = []
        for _ in range(2):
            yy, P1, P2 = y1.clone(), c.out_partials(), c.out_partials()
            c.kr.dots(x1, yy, P1, yy, yy, P2, shift=z, conj1=True)
            xo, om, Prr, Prho, rr = c.out_vec(), c.out_scalar(), c.out_partials(True), c.out_partials(), c.out_vec()
            al = torch.ones(S, dtype=dtype, device=c.dev)
            c.kr.bicg_final(x1, xo, yy, z, z, yy, rr, r0, al, P1, P2, om, Prr, Prho, EPS, False)
            outs.append([t.cpu() for t in (yy, P1, P2, xo, om, Prr, Prho, rr)])
        for a, b in zip(*outs):
            a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
        ref = kref.kry_dots(c.ctx, c.ctx.vec(x1h), c.ctx.vec(y1h), shiftz=c.ctx.vec(zh),
                            E=kref.hp(Eh), conj1=True, x2_is_y1=True, y2_is_y1=True)
        P1 = outs[0][1]
        got = kref.partial_value(P1, c.ctx)[:, :c.nblk].sum(-1)
        c.check({"P1": got}, {"P1": ref["P1"]}, "kry_dots nblk=%d" % c.nblk)
        totals.append((c.nblk, got, ref["P1"][1]))
    for nb, got, bnd in totals[1:]:
        nb0, got0, bnd0 = totals[0]
        assert bool(((got - got0).abs() <= bnd + bnd0).all()), (nb0, nb, (got - got0).abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("S", [1, 3, 257])
@pytest.mark.parametrize("nblk", [1, 7, 64])
@pytest.mark.parametrize("with_nan", [False, True])
def test_kry_status(dev, dtype, S, nblk, with_nan):
    """rnorm = sqrt(sum of the used partials), status = (max rnorm, #unconverged) with the reference's test
    `resid_norm < stop`: a residual exactly equal to its stop value is unconverged, a NaN system is unconverged and
    makes the max +inf; poisoned slots [nblk, 64) are ignored"""
    g = torch.Generator().manual_seed(S * 131 + nblk)
    kr = nk._Kry(_Stub(dtype, S, 1000, pad_len(1000)))
    kr.nblk = nblk
    ctx = kref.Ctx(dtype, S, 1000, nblk)
    P = kref.rand_partials(g, dtype, S, nblk, positive=True)
    ss = kref.partial_value(P, ctx)[:, :nblk].sum(-1)
    fac = torch.where(torch.rand(S, dtype=torch.float64, generator=g) < 0.5, 2.0, 0.5)
    stop = (ss.sqrt() * fac).to(dtype)
    exact = []
    if S >= 3:
        # partials summing to exactly 4.0: rnorm = 2 exactly.  stop 2.0 -> unconverged; the next value up -> converged
        for s, st in ((0, 2.0), (S - 1, float(torch.nextafter(torch.tensor(2.0, dtype=dtype),
                                                              torch.tensor(3.0, dtype=dtype))))):
            P[s, :nblk] = 0
            P[s, nblk - 1] = 1.0
            P[s, 0] += 3.0
            stop[s] = st
            exact.append(s)
    nan_sys = [S // 2] if with_nan else []
    for s in nan_sys:
        P[s, 0] = math.nan
    mx, nbad = kr.check_status(P.to(DEV), stop.to(DEV))
    rn = kr.rnorm.cpu()
    ref = kref.kry_status(ctx, P, stop)["rnorm"]
    fin = torch.ones(S, dtype=torch.bool)
    fin[nan_sys] = False
    assert bool(torch.isnan(rn[~fin]).all())
    kref.check({"rnorm": rn[fin]}, {"rnorm": (ref[0][fin], ref[1][fin])}, dtype, what="kry_status")
    for s in exact:
        assert rn[s].item() == 2.0
    want_mx, want_cnt = kref.status_of(rn, stop)
    assert mx == want_mx and nbad == want_cnt, (mx, nbad, want_mx, want_cnt)
    # the same count from the reference norms: every generic system is a factor 2 away from its stop value
    ref_cnt = int((~fin).sum()) + int((~(ref[0][fin] < kref.hp(stop)[fin])).sum())
    assert nbad == ref_cnt
    if exact:
        assert nbad >= 1
    if with_nan:
        assert mx == math.inf
