"""-m gpu: every entry point of xk_lsmr.hip (xk_lsmr_init, xk_lsmr_bidiag in both halves, xk_lsmr_update) in all four
dtypes, against tests/lsmr_ref.py within its bounds.

Inputs are those of `lsmr_ref.Case` (the configurations tests/test_lsmr_ref.py plants its faults at): N below, at and
off the 16 B vector width, one block and many, S = 1 and many; the other side of the bidiagonalisation has another
length and block count (m != n for both halves); frozen systems, start slots, systems that meet a zero norm (both
breakdowns), the damping rotation.  Every buffer is NaN-poisoned where the kernel has no business: [npad, ld) of the
vectors, partial slots [nblk, 64), the state slot that is not written, the outputs of frozen systems; all of it must
come back bit-identical, [N, npad) must be zero, inputs must not change, stop codes and flags must be exactly equal and
a second run must give identical bits."""
import math
import pytest
import torch
from tests import krylov_ref as kref
from tests import lsmr_ref as lref
from xitorch_amd import kernels as K

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
        self.c = c = lref.Case(dtype, N, S, extra, nblk, seed=N + S)
        self.env, self.dtype = c.env, dtype
        self.S, self.N, self.ld, self.nblk, self.k = S, N, c.ld, nblk, c.k
        self.what = "[%s N=%d S=%d ld=%d nblk=%d]" % (dtype, N, S, c.ld, nblk)

    def dev(self, t):
        return t.clone().to(DEV)

    def poison_vec(self):
        return torch.full((self.S, self.ld), kref.nan_of(self.dtype), dtype=self.dtype, device=DEV)

    def poison_real(self):
        return kref.poisoned_partials(self.dtype, self.S, real=True).to(DEV)

    def poison_state(self):
        return torch.full((2, self.S, lref.NST), math.nan, dtype=torch.float64, device=DEV)

    def vec(self, t, name):
        """contract of a written vector: [N, npad) zero, [npad, ld) untouched; returns the [0, N) part"""
        t = t.cpu()
        c = self.c
        assert bool((t[:, c.N:c.npad] == 0).all()), "%s %s: [N, npad) not zero" % (name, self.what)
        assert bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t)[:, c.npad:].all()), \
            "%s %s: [npad, ld) written" % (name, self.what)
        return self.env.vec(t)

    def check(self, got, ref, name):
        return lref.check(got, ref, self.dtype, what=name + " " + self.what)


@pytest.mark.parametrize("dtype,cfg", lref.CASES, ids=lref.CASE_IDS)
def test_init(dtype, cfg):
    r = _Run(dtype, cfg)
    c = r.c
    b, Pb = r.dev(c.b), r.dev(c.Pb)
    outs = []
    for _ in range(2):
        uh, state, run = r.poison_vec(), r.poison_state(), r.poison_real()
        K.lsmr_init(b, uh, Pb, state, run, r.S, r.N, r.ld, r.nblk, r.k)
        outs.append((uh, state, run))
    uh, state, run = outs[0]
    for a, bb, n in zip(outs[0], outs[1], ("uh", "state", "run")):
        _same(a, bb, n + " of the second run")
    ref = c.ref_init()
    st = state.cpu()
    assert bool(torch.isnan(st[(r.k + 1) & 1]).all()), "the other state slot was written"
    assert torch.equal(st[r.k & 1][:, lref.FLAG], ref["flag"])
    got = {"uh": r.vec(uh, "uh"), "state": st[r.k & 1], "run": run.cpu()[:, 0]}
    r.check(got, lref.comparable(ref, ["uh", "state", "run"]), "lsmr_init")
    assert bool(torch.isnan(run.cpu()[:, 1:]).all()), "run slots [1, 64) written"
    _same(b, c.b, "b")
    _same(Pb, c.Pb, "Pb")


@pytest.mark.parametrize("half", [0, 1], ids=["u-half", "v-half"])
@pytest.mark.parametrize("dtype,cfg", lref.CASES, ids=lref.CASE_IDS)
def test_bidiag(dtype, cfg, half):
    r = _Run(dtype, cfg)
    c = r.c
    Op, Pin, state = r.dev(c.Op), r.dev(c.Pin), c.state.clone().to(DEV)
    outs = []
    for _ in range(2):
        y = r.dev(c.y)
        if half == 1 and c.first:
            y[c.first, :c.npad] = kref.nan_of(dtype)         # a start step must not read y
        Pout = r.poison_real()
        K.lsmr_bidiag(Op, y, Pin, Pout, state, half, r.S, r.N, r.ld, r.nblk, c.nblk2, r.k)
        outs.append((y, Pout))
    y, Pout = outs[0]
    _same(outs[1][0], y, "y of the second run")
    _same(outs[1][1], Pout, "Pout of the second run")
    ref = c.ref_bidiag(half)
    frozen, zero = ref["frozen"], ref["zero"]
    assert bool(frozen[c.frozen].all()) and bool(zero[c.zero].all())
    yh = y.cpu()
    if half == 1 and c.first:
        # start systems: y was poison and has been overwritten entirely ([N, npad) comes from Op's zeros)
        pass
    r.check({"y": r.vec(y, "y")}, lref.comparable(ref, ["y"]), "lsmr_bidiag")
    skip = frozen | zero
    if bool(skip.any()):
        _same(yh[skip], c.y[skip], "y of a frozen / zero-norm system")
    P = Pout.cpu()
    assert bool(torch.isnan(P[:, r.nblk:]).all()), "Pout slots [nblk, 64) written"
    assert bool(torch.isnan(P[frozen]).all()), "Pout of a frozen system written"
    live = ~frozen
    assert bool(torch.isfinite(P[live][:, :r.nblk]).all())
    assert bool((P[zero][:, :r.nblk] == 0).all()), "a zero norm must leave zero partials"
    r.check({"Pout": P[live][:, :r.nblk].double().sum(-1)}, lref.comparable(ref, ["Pout"], live), "lsmr_bidiag Pout")
    for t, h, n in ((Op, c.Op, "Op"), (Pin, c.Pin, "Pin"), (state, c.state, "state")):
        _same(t, h, n)


@pytest.mark.parametrize("dtype,cfg", lref.CASES, ids=lref.CASE_IDS)
def test_update(dtype, cfg):
    r = _Run(dtype, cfg)
    c = r.c
    vh, Pu, Pv, Pxin = r.dev(c.vh), r.dev(c.Pu), r.dev(c.Pv), r.dev(c.Pxin)
    outs = []
    for _ in range(2):
        h, hbar, x = r.dev(c.h), r.dev(c.hbar), r.dev(c.x)
        if c.first:
            h[c.first, :c.npad] = kref.nan_of(dtype)         # a start step must not read h
        state = c.state.clone().to(DEV)
        Pxout, run = r.poison_real(), r.poison_real()
        K.lsmr_update(vh, h, hbar, x, Pu, Pv, Pxin, Pxout, state, run, r.S, r.N, r.ld, r.nblk, c.nblk2, r.k,
                      **lref.TOLS)
        outs.append((h, hbar, x, state, Pxout, run))
    for a, b, n in zip(outs[0], outs[1], ("h", "hbar", "x", "state", "Pxout", "run")):
        _same(a, b, n + " of the second run")
    h, hbar, x, state, Pxout, run = outs[0]
    ref = c.ref_update()
    frozen, start, reg = ref["frozen"], ref["start"], ref["reg"]
    assert bool(frozen[c.frozen].all()) and bool(start[c.first].all())
    st = state.cpu()
    _same(st[r.k & 1], c.state[r.k & 1], "the state slot read")
    got = {"h": r.vec(h, "h"), "hbar": r.vec(hbar, "hbar"), "x": r.vec(x, "x"), "state": st[(r.k + 1) & 1]}
    r.check(got, lref.comparable(ref, ["h", "hbar", "x", "state"]), "lsmr_update")
    want = ref["state"][0]
    for i in (lref.FLAG, lref.ITN):
        assert torch.equal(st[(r.k + 1) & 1][:, i], want[:, i]), "stop codes / step counts must be exactly equal"
    flags = st[(r.k + 1) & 1][:, lref.FLAG]
    assert bool((flags[c.zero_b] == 5).all()) and bool((flags[c.zero_a] == 4).all()) and bool((flags[c.frozen] == 2).all())
    if c.zero:
        assert bool((r.env.vec(h.cpu())[c.zero] == 0).all()), "a zero norm must leave h = 0, not vh / 0"
    untouched = ~reg
    if bool(untouched.any()):
        _same(hbar.cpu()[untouched], c.hbar[untouched], "hbar of a frozen / start system")
        _same(x.cpu()[untouched], c.x[untouched], "x of a frozen / start system")
    if bool(frozen.any()):
        _same(h.cpu()[frozen], c.h[frozen], "h of a frozen system")
    P, R = Pxout.cpu(), run.cpu()
    assert bool(torch.isnan(P[:, r.nblk:]).all()) and bool(torch.isnan(P[~reg]).all()), "Pxout written out of place"
    r.check({"Pxout": P[reg][:, :r.nblk].double().sum(-1)}, lref.comparable(ref, ["Pxout"], reg), "lsmr_update Pxout")
    assert bool(torch.isnan(R[:, 1:]).all()) and bool(torch.isnan(R[frozen][:, 0]).all()), "run written out of place"
    assert torch.equal(R[~frozen][:, 0].double(), ref["run"][0][~frozen]), "run flags must be exactly equal"
    for t, hh, n in ((vh, c.vh, "vh"), (Pu, c.Pu, "Pu"), (Pv, c.Pv, "Pv"), (Pxin, c.Pxin, "Pxin")):
        _same(t, hh, n)


def test_worst_ratio_report():
    """(runs last in this file) the largest |kernel - reference| / bound seen, per dtype"""
    for d, w in sorted(kref.WORST.items(), key=lambda kv: str(kv[0])):
        print("lsmr kernels: worst error / bound for %s: %.3f" % (d, w))
