"""-m gpu: every entry point of xk_minres.hip (xk_minres_init, xk_minres_lanczos, xk_minres_update) and the
xk_kry_dots product MINRES takes alpha from, in all four dtypes, against tests/minres_ref.py within its bounds.

Inputs are those of `minres_ref.Case` (the configurations tests/test_minres_ref.py plants its faults at): N below, at
and off the 16 B vector width, one block and many, S = 1 and many; frozen systems, first steps, a system frozen by
beta_new = 0 and one whose <r2, P r2> is negative (the preconditioner flag).  Every buffer is NaN-poisoned where the
kernel has no business: [npad, ld) of the vectors, partial slots [nblk, 64), the state slot that is not written, the
outputs of frozen systems; all of it must come back bit-identical, and inputs must not change."""
import math
import pytest
import torch
from tests import krylov_ref as kref
from tests import minres_ref as mref
from xitorch_amd import kernels as K
from xitorch_amd.linalg import native_krylov as nk

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), "%s changed" % what


class _Run:
    def __init__(self, dtype, cfg):
        N, S, extra, nblk = cfg
        self.c = c = mref.Case(dtype, N, S, extra, nblk, seed=N + S)
        self.env, self.dtype = c.env, dtype
        self.S, self.N, self.ld, self.nblk, self.k = S, N, c.ld, nblk, c.k
        self.what = "[%s N=%d S=%d ld=%d nblk=%d]" % (dtype, N, S, c.ld, nblk)

    def dev(self, t):
        return t.clone().to(DEV)

    def poison_vec(self):
        return torch.full((self.S, self.ld), kref.nan_of(self.dtype), dtype=self.dtype, device=DEV)

    def poison_real(self):
        return kref.poisoned_partials(self.dtype, self.S, real=True).to(DEV)

    def vec(self, t, name):
        """contract of a written vector: [N, npad) zero, [npad, ld) untouched; returns the [0, N) part"""
        t = t.cpu()
        c = self.c
        assert bool((t[:, c.N:c.npad] == 0).all()), "%s %s: [N, npad) not zero" % (name, self.what)
        assert bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t)[:, c.npad:].all()), \
            "%s %s: [npad, ld) written" % (name, self.what)
        return self.env.vec(t)

    def check(self, got, ref, name):
        return mref.check(got, ref, self.dtype, what=name + " " + self.what)


def _stub_kry(r):
    class _Stub:
        S, N, ld, dtype = r.S, r.N, r.ld, r.dtype
        rdtype = kref.REAL_OF[r.dtype]
        cplx = r.dtype.is_complex
        device = DEV
        E = None
        vec_elems = kref.VEC_ELEMS[r.dtype]

        def nblk(self):
            return r.nblk
    return nk._Kry(_Stub())


@pytest.mark.parametrize("dtype,cfg", mref.CASES, ids=mref.CASE_IDS)
def test_alpha_product(dtype, cfg):
    r = _Run(dtype, cfg)
    kr = _stub_kry(r)
    P = kref.poisoned_partials(dtype, r.S).to(DEV)
    v, Av = r.dev(r.c.v), r.dev(r.c.Av)
    kr.dots(v, Av, P)
    Pc = P.cpu()
    assert bool(torch.isnan(Pc[:, r.nblk:]).all())
    got, _ = mref.psum_real(r.env, Pc)
    r.check({"alpha": got}, mref.comparable(r.c.ref_alpha_dot(), ["alpha"]), "alpha = Re <v, Av>")
    _same(v, r.c.v, "v")
    _same(Av, r.c.Av, "Av")


@pytest.mark.parametrize("dtype,cfg", mref.CASES, ids=mref.CASE_IDS)
def test_init(dtype, cfg):
    r = _Run(dtype, cfg)
    c = r.c
    y, Pb = r.dev(c.y), r.dev(c.Pdot)
    v = r.poison_vec()
    state = torch.full((2, r.S, mref.NST), math.nan, dtype=torch.float64, device=DEV)
    phi2 = r.poison_real()
    K.minres_init(y, v, Pb, state, phi2, r.S, r.N, r.ld, r.nblk, r.k)
    ref = c.ref_init()
    flag = ref["flag"]
    st = state.cpu()
    assert bool(torch.isnan(st[(r.k + 1) & 1]).all()), "the other state slot was written"
    assert torch.equal(st[r.k & 1][:, mref.FLAG], flag)
    r.check({"v": r.vec(v, "v"), "state": st[r.k & 1]}, mref.comparable(ref, ["v", "state"]), "minres_init")
    p = phi2.cpu()
    assert bool(torch.isnan(p[:, 1:]).all()), "phi2 slots [1, 64) written"
    ok = flag != 2
    r.check({"phi2": p[:, 0][ok]}, mref.comparable(ref, ["phi2"], ok), "minres_init phi2")
    assert bool(torch.isinf(p[:, 0][~ok]).all())
    _same(y, c.y, "y0")
    _same(Pb, c.Pdot, "Pb")


@pytest.mark.parametrize("dtype,cfg", mref.CASES, ids=mref.CASE_IDS)
def test_lanczos(dtype, cfg):
    r = _Run(dtype, cfg)
    c = r.c
    Av, r2, r1, Pa, state = r.dev(c.Av), r.dev(c.r2), r.dev(c.r1), r.dev(c.Palpha), c.state.clone().to(DEV)
    if c.first:
        r1[c.first, :c.npad] = kref.nan_of(dtype)        # a first step must not read r1
    Pbeta = r.poison_real()
    K.minres_lanczos(Av, r2, r1, Pa, state, Pbeta, r.S, r.N, r.ld, r.nblk, r.k)
    ref = c.ref_lanczos()
    frozen = ref["frozen"]
    r.check({"r1": r.vec(r1, "r1")}, mref.comparable(ref, ["r1"]), "minres_lanczos")
    P = Pbeta.cpu()
    assert bool(torch.isnan(P[:, r.nblk:]).all()), "Pbeta slots [nblk, 64) written"
    assert bool(torch.isnan(P[frozen]).all()), "Pbeta of a frozen system written"
    live = ~frozen
    assert bool(torch.isfinite(P[live][:, :r.nblk]).all())
    r.check({"Pbeta": P[live][:, :r.nblk].double().sum(-1)}, mref.comparable(ref, ["Pbeta"], live),
            "minres_lanczos Pbeta")
    for t, h, n in ((Av, c.Av, "Av"), (r2, c.r2, "r2"), (Pa, c.Palpha, "Palpha"), (state, c.state, "state")):
        _same(t, h, n)
    # no partials wanted (the preconditioned driver): same vector, nothing else
    r1b = r.dev(c.r1)
    if c.first:
        r1b[c.first, :c.npad] = kref.nan_of(dtype)
    K.minres_lanczos(Av, r2, r1b, Pa, state, None, r.S, r.N, r.ld, r.nblk, r.k)
    _same(r1b, r1, "r1 without partials")


@pytest.mark.parametrize("dot", [False, True], ids=["own-partials", "dots-partials"])
@pytest.mark.parametrize("dtype,cfg", mref.CASES, ids=mref.CASE_IDS)
def test_update(dtype, cfg, dot):
    r = _Run(dtype, cfg)
    c = r.c
    v, y, w1, w2, x = (r.dev(t) for t in (c.v, c.y, c.w1, c.w2, c.x))
    Pa, Pbh = r.dev(c.Palpha), (c.Pdot if dot else c.Pbeta)
    Pb = r.dev(Pbh)
    state = c.state.clone().to(DEV)
    phi2 = r.poison_real()
    K.minres_update(v, y, w1, w2, x, Pa, Pb, dot, state, phi2, r.S, r.N, r.ld, r.nblk, r.k)
    ref = c.ref_update(dot=dot)
    live, negb = ref["live"], ref["negb"]
    assert bool(negb[c.neg_b].all()) and not bool(live[c.frozen].any())
    st = state.cpu()
    _same(st[r.k & 1], c.state[r.k & 1], "the state slot read")
    got = {"v": r.vec(v, "v"), "w": r.vec(w1, "w"), "x": r.vec(x, "x"), "state": st[(r.k + 1) & 1]}
    r.check(got, mref.comparable(ref, ["v", "w", "x", "state"]), "minres_update")
    flags = st[(r.k + 1) & 1][:, mref.FLAG]
    assert bool((flags[c.zero_b] == 1).all()) and bool((flags[c.neg_b] == 2).all()) and bool((flags[c.frozen] == 1).all())
    if c.zero_b:
        assert bool((r.env.vec(v.cpu())[c.zero_b] == 0).all()), "beta_new = 0 must leave v = 0, not y / eps"
    p = phi2.cpu()
    assert bool(torch.isnan(p[:, 1:]).all()), "phi2 slots [1, 64) written"
    r.check({"phi2": p[:, 0][live]}, mref.comparable(ref, ["phi2"], live), "minres_update phi2")
    assert bool(torch.isinf(p[:, 0][negb]).all())
    assert bool(torch.isnan(p[:, 0][~(live | negb)]).all()), "phi2 of a frozen system written"
    for t, h, n in ((y, c.y, "y"), (w2, c.w2, "w2"), (Pa, c.Palpha, "Palpha"), (Pb, Pbh, "Pbeta")):
        _same(t, h, n)


def test_worst_ratio_report():
    """(runs last in this file) the largest |kernel - reference| / bound seen, per dtype"""
    for d, w in sorted(kref.WORST.items(), key=lambda kv: str(kv[0])):
        print("minres kernels: worst error / bound for %s: %.3f" % (d, w))
