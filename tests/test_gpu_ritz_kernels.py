"""-m gpu: the Ritz eigensolvers K3t (xk_small_eigh_tri_*) and K3g (xk_small_eigh_big_*: one launch per Householder
step, persistent, two-stage, and the automatic choice) against spectra that are known exactly (tests/ritz_cases.py), at
every order where a form changes its path, with wanted counts that cross the LU batches of the inverse iteration,
at scales next to the edge of the range the kernels accept, and bit-reproducibly.

The kernels' self-check sees the tridiagonal level only, so a wrong reduction or back-transformation comes back
unflagged: every bound here is  c k u  times the natural scale, c = FACTOR[form] x the error of LAPACK's ?syevx in the
same precision on the same matrices (ritz_cases.EVX_RATIO, asserted by test_ritz_cases.py).  In-range members must be
unflagged (info == 0), out-of-range ones flagged.

Every call gets T inside a larger NaN-filled allocation (ldt > k, sT > k ldt, nonzero storage offset, NaN strict upper
triangle), a NaN-filled workspace, and NaN / -1 sentinels in lam, Y and info.

Worst ratios measured on an MI355X (profiles/ritz_kernels_worst.json), each as  measured / bound  at the order where
measured / bound is largest; no member of 8336 came back flagged:
  tri       float64  lam 0.571 / 4 (order 7)   res 0.667 / 4 (order 2)   orth 2 / 12 (order 2)   proj 1.33 / 4 (order 2)
  tri       float32  lam 0.714 / 4 (order 7)   res 0.706 / 3 (order 7)   orth 1.5 / 12 (order 7)   proj 0.589 / 2 (order 7)
  step      float64  lam 0.24 / 1 (order 129)   res 0.667 / 4 (order 9)   orth 0.0936 / 1 (order 513)   proj 0.312 / 4 (order 8)
  step      float32  lam 0.5 / 4 (order 8)   res 0.625 / 3 (order 8)   orth 0.709 / 12 (order 9)   proj 0.333 / 2 (order 9)
  persist   float64  lam 0.24 / 1 (order 129)   res 0.438 / 4 (order 8)   orth 0.75 / 12 (order 8)   proj 0.25 / 4 (order 8)
  persist   float32  lam 0.0701 / 1 (order 150)   res 0.347 / 3 (order 8)   orth 0.679 / 12 (order 8)   proj 0.206 / 2 (order 8)
  two_stage float64  lam 0.475 / 2 (order 193)   res 0.142 / 2 (order 150)   orth 0.173 / 8 (order 150)   proj 0.129 / 8 (order 35)
  two_stage float32  lam 0.14 / 2 (order 150)   res 0.214 / 2 (order 193)   orth 0.167 / 6 (order 150)   proj 0.109 / 4 (order 35)
  auto      float64  lam 0.475 / 2 (order 193)   res 0.0762 / 2 (order 385)   orth 0.127 / 8 (order 150)   proj 0.0152 / 2 (order 191)
  auto      float32  lam 0.0701 / 2 (order 150)   res 0.0956 / 2 (order 150)   orth 0.0489 / 6 (order 150)   proj 0.0114 / 2 (order 191)
"""
import json
import os
import pytest
import torch
from xitorch_amd import kernels as K
from xitorch_amd._capi import call, fn, ptr
from tests import jacobi_cases as jc
from tests import ritz_cases as rc

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTYPES = [torch.float64, torch.float32]
NAN = float("nan")
WORST = {}          # (form, dtype name, quantity) -> (ratio / bound, ratio, bound, order): the worst of this run
FLAGGED = {}        # (form, dtype name) -> members that came back flagged where a flag is allowed (ritz_cases.XFLAG)
MEMBERS = {}        # (form, dtype name) -> members checked
XK_ERR_UNSUPPORTED = -2


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _place(Ts, k, dtype, dev):
    """the (k, k) float64 matrices Ts (exact in dtype) as a strided device view inside a NaN-filled allocation"""
    B = len(Ts)
    ldt, off = k + 3, 5
    sT = k * ldt + 7
    buf = torch.full((off + B * sT,), NAN, dtype=dtype)
    Tv = buf.as_strided((B, k, k), (sT, ldt, 1), off)
    low = torch.tril(torch.ones(k, k, dtype=torch.bool))
    for b in range(B):
        Tv[b][low] = Ts[b].to(dtype)[low]
    return buf.to(dev).as_strided((B, k, k), (sT, ldt, 1), off)


def _run(form, Td, k, p, uppest, wg=0):
    """one call of the form on the placed matrices: float64 CPU copies of lam (B, p), Y (B, p, k) and info, plus the
    device outputs themselves"""
    B, dtype, dev = Td.shape[0], Td.dtype, Td.device
    lam = torch.full((B, p), NAN, dtype=dtype, device=dev)
    Y = torch.full((B, p, k), NAN, dtype=dtype, device=dev)
    info = torch.full((B,), -1, dtype=torch.int32, device=dev)
    if form == "tri":
        out = K.small_eigh(Td, k, p, uppest=uppest, method="tri", out=(lam, Y, info))
        assert out[0].data_ptr() == lam.data_ptr() and out[1].data_ptr() == Y.data_ptr()
    else:
        nws = fn("xk_small_eigh_big_workspace_elems")(B, k, wg)
        ws = K._workspace(nws, dtype, dev)
        ws.fill_(NAN)
        call("xk_small_eigh_big", dtype, ptr(Td), ptr(lam), ptr(Y), ptr(ws), nws, ptr(info), B, k, p,
             1 if uppest else 0, Td.stride(1), Td.stride(0), wg, 0, rc.ALGO[form])
    return lam.cpu().double(), Y.cpu().double(), info.cpu(), (lam, Y, info)


def _record(form, dtype, k, r):
    for q, v in r.items():
        if v is None:
            continue
        bnd = rc.bound(form, q, dtype, k)
        key = (form, _name(dtype), q)
        if v / bnd >= WORST.get(key, (-1.0,))[0]:
            WORST[key] = (v / bnd, v, bnd, k)


def _check_exact(form, cases, fams, lam, Y, info, p, uppest, dtype, tag, scale_exp=0):
    """per member: unflagged, finite, ascending, every quantity of ritz_cases.ratios within its bound"""
    for b, c in enumerate(cases):
        t = tag + (fams[b], b)
        k = c.T.shape[0]
        fkey = (form, _name(dtype))
        MEMBERS[fkey] = MEMBERS.get(fkey, 0) + 1
        assert int(info[b]) >= 0, t                                                # the sentinel left: info unwritten
        if int(info[b]) != 0:
            assert fams[b] == "multiple64" and fkey in rc.XFLAG, (t, "flagged", int(info[b]))
            FLAGGED[fkey] = FLAGGED.get(fkey, 0) + 1
            continue
        assert torch.isfinite(lam[b]).all() and torch.isfinite(Y[b]).all(), t      # a sentinel left = an unwritten entry
        assert bool((lam[b, 1:] >= lam[b, :-1]).all()), t
        lb = torch.ldexp(lam[b], torch.tensor(-scale_exp))                         # exact: back to the unscaled case
        r = rc.ratios(c.T, lb, Y[b], c, p, uppest, dtype)
        _record(form, dtype, k, r)
        for q, v in r.items():
            assert v is None or v <= rc.bound(form, q, dtype, k), (t, q, v, rc.bound(form, q, dtype, k))


def _launches(form, k, dtype, B):
    """the (member slice, wg) of the launches that carry a batch of B members: `auto` chooses by batch (B <= 8 / B > 8),
    so it gets the whole batch and its two halves; the hand-over orders of `persist` run with every HANDOVER_WG"""
    if form == "auto":
        return [(slice(0, B), 0), (slice(0, B // 2), 0), (slice(B // 2, B), 0)]
    if form == "persist" and k in rc.handover_orders(dtype):
        return [(slice(0, B), wg) for wg in rc.HANDOVER_WG]
    return [(slice(0, B), 0)]


ITEMS = [(f, k, d) for f in rc.FORMS for d in DTYPES for k in rc.orders(f, d)]


@pytest.mark.parametrize("form,k,dtype", ITEMS, ids=["%s-%d-%s" % (f, k, _name(d)) for f, k, d in ITEMS])
def test_exact_spectra(dev, form, k, dtype):
    """the nine families as the batch of one launch, for every wanted count and both ends of the spectrum"""
    cases = rc.cases(k, dtype)
    Td = _place([c.T for c in cases], k, dtype, dev)
    B = len(cases)
    assert B == 9
    for sl, wg in _launches(form, k, dtype, B):
        for p in rc.wanted_counts(form, k, dtype):
            for uppest in (False, True):
                lam, Y, info, _ = _run(form, Td[sl], k, p, uppest, wg)
                _check_exact(form, cases[sl], rc.FAMILIES[sl], lam, Y, info, p, uppest, dtype, (form, k, p, uppest, wg))


def test_two_stage_refuses_what_its_band_does_not_fit(dev):
    k, dtype = rc.TWO_STAGE_REFUSED
    Td = _place([rc.case("spread", k, dtype).T], k, dtype, dev)
    lam = torch.full((1, 6), NAN, dtype=dtype, device=dev)
    Y = torch.full((1, 6, k), NAN, dtype=dtype, device=dev)
    info = torch.full((1,), -1, dtype=torch.int32, device=dev)
    nws = fn("xk_small_eigh_big_workspace_elems")(1, k, 0)
    ws = K._workspace(nws, dtype, dev)
    code = call("xk_small_eigh_big", dtype, ptr(Td), ptr(lam), ptr(Y), ptr(ws), nws, ptr(info), 1, k, 6, 0,
                Td.stride(1), Td.stride(0), 0, 0, rc.ALGO["two_stage"], raw=True)
    assert code == XK_ERR_UNSUPPORTED
    assert int(info[0]) == -1 and bool(torch.isnan(lam).all())          # nothing was launched


@pytest.mark.parametrize("form", rc.FORMS)
def test_batch_of_70(dev, form):
    """70 distinct members in one launch: more workgroups than one per family, every batch pitch"""
    k = rc.BATCH70_ORDER[form]
    for dtype in DTYPES:
        cases = jc.batch70(k, dtype)
        fams = [jc.FAMILIES[i % len(jc.FAMILIES)] for i in range(70)]
        Td = _place([c.T for c in cases], k, dtype, dev)
        pw = 16 if form == "tri" else (rc.cross_p(k, dtype) or 16)
        for p, uppest in ((6, False), (pw, True)):
            lam, Y, info, _ = _run(form, Td, k, p, uppest)
            _check_exact(form, cases, fams, lam, Y, info, p, uppest, dtype, (form, k, p, uppest, "of 70"))


@pytest.mark.parametrize("form", rc.FORMS)
def test_scale(dev, form):
    """T 2^e: inside the range of tri_scale_in_range the bounds of e = 0 hold and nothing is flagged, even where
    alpha^2 + sigma and e^2 come close to leaving the floating-point range; outside it every member is flagged"""
    for dtype in DTYPES:
        for k in rc.scale_orders(form, dtype):
            cases = [rc.case(f, k, dtype) for f in rc.SCALE_FAMILIES]
            p = rc.scale_p(form, k, dtype)
            for side in ("in", "out"):
                for e in rc.SCALE_EXPONENTS[dtype][side]:
                    Td = _place([torch.ldexp(c.T, torch.tensor(e)) for c in cases], k, dtype, dev)
                    for uppest in (False, True):
                        lam, Y, info, _ = _run(form, Td, k, p, uppest)
                        tag = (form, "scale", e, k, p, uppest)
                        if side == "in":
                            _check_exact(form, cases, rc.SCALE_FAMILIES, lam, Y, info, p, uppest, dtype, tag, scale_exp=e)
                        else:
                            assert bool((info != 0).all()) and bool((info != -1).all()), (tag, info.tolist())


GENERIC = [(f, k) for f in rc.FORMS for k in rc.GENERIC_ORDERS[f]]


@pytest.mark.parametrize("form,k", GENERIC, ids=["%s-%d" % fk for fk in GENERIC])
def test_generic_dense(dev, form, k):
    """(R + R^T) / 2 against float64 LAPACK on the rounded matrix, in the same units and within the same bounds"""
    B = 3 if k <= 512 else 2
    for dtype in DTYPES:
        T = jc.generic(B, k, dtype, seed=4000 + k)
        lam_ref = torch.linalg.eigvalsh(T)
        Td = _place(list(T), k, dtype, dev)
        ps = rc.wanted_counts(form, k, dtype)
        for p, uppest in ((rc.scale_p(form, k, dtype), False), (ps[-1], True)):
            sl = slice(k - p, k) if uppest else slice(0, p)
            lam, Y, info, _ = _run(form, Td, k, p, uppest)
            tag = (form, k, p, uppest, _name(dtype))
            assert info.tolist() == [0] * B, (tag, info.tolist())
            assert torch.isfinite(lam).all() and torch.isfinite(Y).all(), tag
            assert bool((lam[:, 1:] >= lam[:, :-1]).all()), tag
            for b in range(B):
                r = rc.ratios_generic(T[b], lam[b], Y[b], lam_ref[b, sl], dtype)
                _record(form, dtype, k, r)
                for q, v in r.items():
                    assert v <= rc.bound(form, q, dtype, k), (tag, b, q, v, rc.bound(form, q, dtype, k))


@pytest.mark.parametrize("form", rc.FORMS)
def test_two_calls_give_equal_bits(dev, form):
    for dtype in DTYPES:
        for k in rc.EQUAL_BITS_ORDERS[form][dtype]:
            Ts = [c.T for c in rc.cases(k, dtype)] + list(jc.generic(2, k, dtype, 5000 + k))
            Td = _place(Ts, k, dtype, dev)
            p = rc.scale_p(form, k, dtype)
            a = _run(form, Td, k, p, False)[3]
            b = _run(form, Td, k, p, False)[3]
            for x, y in zip(a, b):
                assert torch.equal(x, y), (form, k, _name(dtype))


def test_zz_worst_ratios():
    """the kernels' worst error per (form, dtype, quantity) of this run, in the units of jacobi_cases.ratios, next to
    its bound, and the flagged members; written as JSON where XK_RITZ_WORST_JSON points"""
    rep = {"%s/%s/%s" % key: {"ratio": round(v, 4), "bound": bnd, "order": k}
           for key, (_, v, bnd, k) in sorted(WORST.items())}
    flags = {"%s/%s" % key: {"members": n, "flagged": FLAGGED.get(key, 0)} for key, n in sorted(MEMBERS.items())}
    print("ritz kernels worst ratios:", json.dumps(rep))
    print("ritz kernels flagged members:", json.dumps(flags))
    path = os.environ.get("XK_RITZ_WORST_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"worst": rep, "flags": flags}, f, indent=1)
    for key, (frac, v, bnd, k) in WORST.items():
        assert frac <= 1.0, (key, v, bnd, k)
    for key, n in FLAGGED.items():
        assert key in rc.XFLAG, (key, n)
